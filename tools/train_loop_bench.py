#!/usr/bin/env python3
"""What a training loop that includes its data achieves: ms/step of `driver.train_one_epoch` by the loader that feeds it.

    python tools/train_loop_bench.py [--samples 4096] [--tracks 512] [--out profiles/train_loop_bench.json]

A synthetic split is written to a temporary directory -- per-id `.pt` files in the reference's layout and, in a second tree, a bf16
pack (`--max_v_frames 30`, stride 2.5 over 240 s: T_a = 96, `--dim_input 256`, bf16 compute, `--batch_size_train 64`) -- and every
leg runs in a process of its own under `timeout`: one warm-up epoch, then one timed epoch of samples / 64 steps (`ms_per_step`:
the whole epoch, the loader's start included; `ms_per_step_second_half`: from the hand-out of the middle batch to the end).

    files_w16          DataLoader over the per-id files, 16 workers
    packed_w16 / _w0   DataLoader over the packed store, 16 workers / in the main process
    device             DeviceLoader over a DeviceFeatureStore of the pack (raw bf16 on the device); also the store's build time and
                       bytes, made_gather_batch alone (events around 20 launches, median of 5) and the host's time per store.gather call
    device_files       the same over a store built from the per-id files (f32 on the device)
    device_parent_loop the device loader under the loop body as it was BEFORE the host reads left it (a copy below: float() of the
                       losses and iou.cpu() every step), so the two changes can be told apart
    floor              `train_step` alone on one resident batch, called as the loop calls it

One JSON object; nothing is asserted.  The files have just been written, so the host loaders read them from the page cache."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = {"files_w16": ("files", 16, 0), "packed_w16": ("packed", 16, 0), "packed_w0": ("packed", 0, 0), "device": ("packed", 0, 1),
        "device_files": ("files", 0, 1), "device_parent_loop": ("packed", 0, 1), "floor": ("packed", 0, 1)}
COLS = "video_id,music_id,video_start,video_end,music_start,music_end,music_total_duration,video_segment_duration,music_segment_duration," \
       "music_path,video_total_duration,video_width,video_height,video_total_frames,video_frame_rate,video_category"


def write_split(root: str, n: int, tracks: int) -> None:
    import numpy as np
    import torch
    from mgsv_amd import feature_store as fs
    rng = np.random.default_rng(0)
    g = torch.Generator().manual_seed(0)
    dirs = {}
    for tree in ("files", "packed"):
        for kind, sub in (("vit", "vit_feature1"), ("ast", "ast_feature2p5")):
            dirs[tree, kind] = os.path.join(root, tree, sub)
            os.makedirs(dirs[tree, kind])
    for kind in ("vit", "ast"):
        os.makedirs(os.path.join(dirs["files", kind], f"{kind}_feature")); os.makedirs(os.path.join(dirs["files", kind], f"{kind}_mask"))
    durs = rng.uniform(60, 240, size=tracks)
    with open(os.path.join(root, "train.csv"), "w") as f:
        f.write(COLS + "\n")
        for i in range(n):
            t = int(rng.integers(0, tracks))
            vd = float(rng.uniform(8, 30))
            ms = float(rng.uniform(0, durs[t] - vd - 1))
            f.write(f"{100000 + i},m{t},0.0,{vd:.3f},{ms:.3f},{ms + vd:.3f},{durs[t]:.3f},{vd:.3f},{vd:.3f},/x.mp3,{vd:.2f},720,1280,300,30,Cat\n")
            torch.save(torch.randn(30, 512, generator=g), os.path.join(dirs["files", "vit"], "vit_feature", f"{100000 + i}.pt"))
            torch.save((torch.arange(30) < max(1, min(30, round(vd)))).float(), os.path.join(dirs["files", "vit"], "vit_mask", f"{100000 + i}.pt"))
    for t in range(tracks):
        torch.save(torch.randn(96, 768, generator=g), os.path.join(dirs["files", "ast"], "ast_feature", f"m{t}.pt"))
        torch.save((torch.arange(96) < max(1, min(96, round(durs[t] / 2.5)))).float(), os.path.join(dirs["files", "ast"], "ast_mask", f"m{t}.pt"))
    fs.pack(dirs["files", "vit"], "vit", [str(100000 + i) for i in range(n)], os.path.join(dirs["packed", "vit"], "vit.made"), "bf16")
    fs.pack(dirs["files", "ast"], "ast", [f"m{t}" for t in range(tracks)], os.path.join(dirs["packed", "ast"], "ast.made"), "bf16")


def parent_train_one_epoch(epoch, args, model, loader, device, logger, total_step, warmup_steps):
    """driver.train_one_epoch's fused-step body as it was before the host reads left the loop (leg device_parent_loop)."""
    import torch
    from mgsv_amd import driver
    from mgsv_amd.utils.util_test import IoU_metrics
    model.train()
    ious = []
    t0 = time.time()
    meter = {"loss": 0.0, "ret": 0.0, "loc": 0.0, "n": 0}
    for step, (data_map, meta_map, spans_target) in enumerate(loader):
        ff, sf, fm, sm, tg, vdur = driver._to_device(data_map, meta_map, spans_target, device)
        fac = driver.lr_factor(args, args.total_step, warmup_steps, total_step)
        trn = model._trainer_ready()
        wr = torch.tensor([args.ret_loss_weight], device=device)
        wl = torch.tensor([args.loc_loss_weight], device=device)
        model._train_seed += 1
        o = trn.train_step(ff, sf, fm, sm, tg, seed=model._train_seed, lrs=(args.matching_lr * fac, args.matching_lr * fac, args.detection_lr * fac),
                           max_grad_norm=args.max_grad_norm, w_ret=wr, w_loc=wl, dist=None, v_duration=vdur)
        ret, loc = o["retrieval_loss"][0] * args.ret_loss_weight, o["localization_loss"][0] * args.loc_loss_weight
        iou = driver._batch_iou(args, model, o, meta_map, device)
        ious.extend(iou.cpu().tolist())
        args.total_step += 1
        b = ff.shape[0]
        meter["loss"] += float(ret + loc) * b; meter["ret"] += float(ret) * b; meter["loc"] += float(loc) * b; meter["n"] += b
        if args.rank == 0 and (step + 1) % max(1, len(loader) // max(args.num_display, 1)) == 0:
            logger.info(f"Train [{epoch}/{args.epochs}, {step + 1}/{len(loader)}] loss {meter['loss'] / meter['n']:.4f} "
                        f"ret {meter['ret'] / meter['n']:.4f} loc {meter['loc'] / meter['n']:.4f} lr x{fac:.3f} "
                        f"{(time.time() - t0) / (step + 1) * 1e3:.1f} ms/step")
    return meter["loss"] / max(meter["n"], 1), IoU_metrics(ious) if ious else {"mIoU": 0.0}


class Stamped:
    """a loader that notes when it hands out every batch"""

    def __init__(self, loader):
        self.loader, self.at = loader, []

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        self.at = []
        for b in self.loader:
            self.at.append(time.time())
            yield b


def run_leg(leg: str, root: str) -> dict:
    import statistics
    import torch
    from mgsv_amd import driver
    tree, workers, dev_feats = LEGS[leg]
    args = driver.parse_option(["--name", leg, "--do_train", "--epochs", "2", "--max_v_frames", "30", "--stride", "2.5", "--max_m_duration", "240",
                                "--dim_input", "256", "--compute_dtype", "bf16", "--batch_size_train", "64", "--num_workers", str(workers),
                                "--frozen_feature_path", os.path.join(root, tree), "--train_csv", os.path.join(root, "train.csv"),
                                "--output_dir", os.path.join(root, "logs"), "--save_model", "0", "--tb_writer", "0",
                                "--device_features", str(dev_feats)])
    device, dist, logger = driver.init_runtime(args)
    model = driver.build_model(args, device, logger)
    t0 = time.time()
    loader, n, _ = driver.make_loader(args.train_csv, args, args.batch_size_train, True, 1, 0)
    out = {"leg": leg, "source": tree, "num_workers": workers, "device_features": dev_feats, "samples": n, "steps": len(loader),
           "loader_build_s": round(time.time() - t0, 3)}
    store = loader.store if dev_feats else None
    loader = Stamped(loader)
    total_step = len(loader) * args.epochs
    warmup_steps = int(total_step * args.warmup_rate)
    args.total_step = 0

    def sync():
        torch.cuda.synchronize(device)

    if leg == "floor":
        data_map, meta_map, spans_target = next(iter(loader))
        ff, sf, fm, sm, tg, vdur = driver._to_device(data_map, meta_map, spans_target, device)
        trn = model._trainer_ready()

        def steps(k):
            for _ in range(k):
                fac = driver.lr_factor(args, args.total_step, warmup_steps, total_step)
                wr = torch.tensor([args.ret_loss_weight], device=device)
                wl = torch.tensor([args.loc_loss_weight], device=device)
                model._train_seed += 1
                trn.train_step(ff, sf, fm, sm, tg, seed=model._train_seed, lrs=(args.matching_lr * fac, args.matching_lr * fac, args.detection_lr * fac),
                               max_grad_norm=args.max_grad_norm, w_ret=wr, w_loc=wl, dist=None, v_duration=vdur)
                args.total_step += 1
        steps(len(loader)); sync()
        t0 = time.time(); steps(len(loader)); sync()
        out["ms_per_step"] = round((time.time() - t0) / len(loader) * 1e3, 3)
        return out

    def epoch(e):
        if leg == "device_parent_loop":
            return parent_train_one_epoch(e, args, model, loader, device, logger, total_step, warmup_steps)
        return driver.train_one_epoch(e, args, model, loader, None, device, dist, logger, total_step, warmup_steps)

    epoch(1); sync()
    t0 = time.time()
    loss, _ = epoch(2); sync()
    t1 = time.time()
    out["ms_per_step"] = round((t1 - t0) / len(loader) * 1e3, 3)
    out["pairs_per_s"] = round(len(loader) * 64 / (t1 - t0), 1)
    half = len(loader) // 2                                       # from the moment batch `half` was handed out: without the workers' start
    out["ms_per_step_second_half"] = round((t1 - loader.at[half]) / (len(loader) - half) * 1e3, 3)
    out["first_batch_s"] = round(loader.at[0] - t0, 3)
    out["train_loss"] = loss
    if dev_feats:
        from mgsv_amd import _lib, ops
        out["store"] = {"build_s": round(store.build_seconds, 3), "bytes": store.nbytes, "videos": int(store.t["video_feats"].shape[0]),
                        "tracks": int(store.t["music_feats"].shape[0]), "feature_dtype": str(store.t["video_feats"].dtype)}
        index = torch.randperm(n, device=device)[:64].to(torch.int32)
        # the launch alone: outputs and descriptors prepared once, 20 launches between two events (the host issues them faster than
        # they run), median of 5
        arrays = store._arrays()
        dst = [torch.empty((64,) + tuple(shape), dtype=torch.float32, device=device) for _, _, shape in arrays]
        ga = ops.gather_batch_args([(src, row, d) for (src, row, _), d in zip(arrays, dst)], index, n)
        stream = torch.cuda.current_stream().cuda_stream
        launch = _lib.lib().made_gather_batch
        _lib.check(launch(ga, stream), "made_gather_batch"); sync()
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                launch(ga, stream)
            b.record(); sync()
            ms.append(a.elapsed_time(b) / 20)
        # and as the loader calls it: eight fresh tensors and the descriptors built per call
        t0 = time.time()
        for _ in range(200):
            store.gather(index, ())
        host_us = (time.time() - t0) / 200 * 1e6
        sync()
        written = sum(t.numel() * 4 for t in dst)
        read = sum(d.numel() * src.element_size() for (src, _, _), d in zip(arrays, dst))
        med = statistics.median(ms)
        out["gather_batch"] = {"B": 64, "launch_ms": round(med, 5), "launch_ms_runs": [round(x, 5) for x in ms], "bytes_written": written,
                               "bytes_read_at_most": read, "gb_per_s": round((written + read) / med / 1e6, 1),
                               "store_gather_host_us_per_call": round(host_us, 1)}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--samples", type=int, default=4096)
    p.add_argument("--tracks", type=int, default=512)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_loop_bench.json"))
    p.add_argument("--leg_timeout", type=int, default=240)
    p.add_argument("--leg", default=None)
    p.add_argument("--root", default=None)
    a = p.parse_args()
    if a.leg:
        print("LEG " + json.dumps(run_leg(a.leg, a.root)), flush=True)
        return
    root = tempfile.mkdtemp(prefix="train_loop_bench_")
    try:
        t0 = time.time()
        write_split(root, a.samples, a.tracks)
        res = {"metric": "train_loop_bench", "samples": a.samples, "tracks": a.tracks, "batch": 64, "T_v": 30, "T_a": 96, "dim_input": 256,
               "compute_dtype": "bf16", "split_written_s": round(time.time() - t0, 1), "legs": {}}
        print(f"split written in {res['split_written_s']} s", flush=True)
        for leg in LEGS:
            r = subprocess.run(["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--root", root],
                               capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("LEG ")]
            if r.returncode != 0 or not line:
                res["legs"][leg] = {"failed": r.returncode, "stderr_tail": r.stderr[-400:]}
                print(f"{leg}: exit status {r.returncode}; no further leg is started", flush=True)
                break
            res["legs"][leg] = json.loads(line[-1][4:])
            print(leg, json.dumps(res["legs"][leg]), flush=True)
        L = res["legs"]
        if all("ms_per_step" in L.get(k, {}) for k in LEGS):
            floor = L["floor"]["ms_per_step"]
            res["ratios"] = {k + "_over_floor": round(L[k]["ms_per_step"] / floor, 3) for k in LEGS if k != "floor"}
            res["ratios"]["files_w16_over_device"] = round(L["files_w16"]["ms_per_step"] / L["device"]["ms_per_step"], 3)
            res["ratios"]["packed_w16_over_device"] = round(L["packed_w16"]["ms_per_step"] / L["device"]["ms_per_step"], 3)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
