"""Fingerprint of one training step, or of the inference entry points, for changes that must not move an operation (docs/EXPERIMENTS.md 3h,
3h-2, 3h-3): run it once per tree on ONE build of the library and compare the files.
  python tools/step_fingerprint.py record --tree PATH --config NAME --out F.json [--runs 5]    (a fresh process, one GPU; PATH holds mgsv_amd/)
  python tools/step_fingerprint.py compare PARENT.json NEW.json                                 (no GPU; exit status 1 when something differs)
  python tools/step_fingerprint.py record-infer --tree PATH --out F.json                        (every inference entry, one process)
  python tools/step_fingerprint.py compare-infer PARENT.json PARENT2.json NEW.json              (PARENT2: the parent recorded a second time)
F.json of `record`: (a) `ops`: the recorded step's (kind, function, stream, grid) with functions and streams numbered by first appearance,
recorded with the tape's duplicate-dependency pass off and in program order, so that every wait the Python issues is there; `foreign`: the
framework kernels inside the step (such a step cannot be replayed: recorded with MADE_TAPE_CHECK=0); `counts`: the default tape's (launches,
event operations, others).  (b) `forward`: SHA-256 per tensor of forward_train's dictionary (seed 7), valid rows only where kernels skip padded
rows.  (c) `backward`: SHA-256 of the decoder's data-gradient chain after one eager train_step (seed 7, learning rates 0); F.npy: flat_grad of
`runs` such steps (f32 atomic adds in a free order: compared as distributions, see compare()).
F.json of `record-infer`: per entry of infer_entries() the same `ops` and `foreign` of the call under LaunchTape.record(check=False) (the tape
mirrors wait_stream / wait_event / Event.record, so a moved wait shows; it is never replayed) and `out`: SHA-256 per tensor of the result;
F.npz: the tensors themselves, for those the parent does not reproduce (compare_infer())."""
import argparse, dataclasses, hashlib, itertools, json, os, sys
import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (4, 20, 40)
CONFIGS = {  # name: (dtype, (B, T_v, T_a), overrides of cfg_headline())
    "headline": ("bf16", (64, 30, 512), {}),
    "f32": ("f32", SMALL, {}),
    "prenorm": ("bf16", SMALL, dict(detr_pre_norm=True)),
    "xpool": ("bf16", SMALL, dict(moment_query_type="xpool", vmr_fusion="XA-video-music", vmr_loss="single")),
    "q2": ("bf16", SMALL, dict(num_moment_queries=2)),
    "regression": ("bf16", SMALL, dict(mml_localization="regression")),
    "ca": ("bf16", SMALL, dict(mml_fusion="CA", contrastive_align_loss=1, audio_short_cut=1, moment_loss=1, predict_center=1)),
    "enc0": ("bf16", SMALL, dict(detr_enc_layers=0)),
}


def setup(a):
    os.environ["MADE_DEBUG_VARIANTS"] = "1"                    # (measurement knobs are honoured only under this switch)
    os.environ["MADE_TAPE_CHECK"] = "0"
    os.environ.setdefault("MADE_LIB_PATH", os.path.join(HERE, "mgsv_amd", "libmade_hip.so"))   # the build is always this tree's
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    return torch, torch.device("cuda", 0)


def sha(x, valid=None) -> str:
    import torch
    x = x.detach() if valid is None else x.detach()[valid]
    return hashlib.sha256(x.contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def numbered(ops) -> list:
    fns, sts = {}, {}
    return [(k, fns.setdefault(fn, len(fns)), sts.setdefault(st, len(sts)), grid) for k, fn, st, grid in ops]


def valid_rows(cfg, fm, sm) -> dict:
    """padded rows of these are skipped by design and hold whatever the buffer held"""
    import torch
    fm, sm = fm.bool(), sm.bool()
    return dict(frame_feats=fm, proj_vid_mem=fm, segment_feats=sm, memory=torch.cat([fm, sm], 1) if "concat" in cfg.mml_fusion else sm)


def record(a) -> None:
    torch, dev = setup(a)
    from mgsv_amd import synth
    from mgsv_amd.config import cfg_headline
    from mgsv_amd.trainer import MadeTrainer
    dtype, (B, Tv, Ta), over = CONFIGS[a.config]
    cfg = dataclasses.replace(cfg_headline(), **over)
    trn = MadeTrainer(cfg, synth.make_state_dict(cfg, seed=0), device=dev, dtype=dtype)
    t = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_inputs(cfg, B, Tv, Ta, seed=1).items() if isinstance(v, np.ndarray)}
    batch = (t["frame_feats"], t["segment_feats"], t["frame_masks"], t["segment_masks"], t["spans_target"])

    # (b)
    valid = valid_rows(cfg, batch[2], batch[3])
    out = trn.forward_train(*batch, seed=7, v_duration=t["v_duration"])
    torch.cuda.synchronize()
    res = dict(tree=os.path.abspath(a.tree), config=a.config, forward={k: sha(v, valid.get(k)) for k, v in out.items() if isinstance(v, torch.Tensor)})

    # (c) the chain's buffers are zeroed first: a configuration writes only the parts it uses
    tw = trn._train_buffers(B, Tv, Ta)
    chain = {"dchain": tw["dchain"], **{k: v for k, v in tw["dstack"].items() if k.startswith("g_") or k == "dt1q"}}
    for v in chain.values():
        v.zero_()
    grads = np.empty((a.runs, trn.flat_grad.numel()), np.float32)
    for r in range(a.runs):
        trn.train_step(*batch, seed=7, lrs=(0.0, 0.0, 0.0), v_duration=t["v_duration"])
        torch.cuda.synchronize()
        grads[r] = trn.flat_grad.cpu().numpy()
        if r == 0:
            res["backward"] = {k: sha(v) for k, v in chain.items()}
    np.save(os.path.splitext(a.out)[0] + ".npy", grads)
    res["params"] = [(k, trn._offs[k], trn.master[k].numel()) for k in trn.param_names]

    # (a)
    def tape(**env):
        for k in ("MADE_TAPE_NO_DEDUP", "MADE_TAPE_INTERLEAVE"):
            os.environ.pop(k, None)
        os.environ.update(env)
        return trn.capture_train_step(*batch, v_duration=t["v_duration"], mode="tape")
    g = tape(MADE_TAPE_NO_DEDUP="1", MADE_TAPE_INTERLEAVE="0")
    res["ops"] = numbered(g.tape.ops())
    res["foreign"] = list(g.tape.foreign_ops)
    g.close()
    g = tape()
    res["counts"] = g.tape.counts()
    g.close()
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(f"{a.config} [{a.tree}]: {len(res['ops'])} operations without the dedup pass, {len(res['foreign'])} framework kernels; default tape "
          f"{res['counts']} = {sum(res['counts'])}")


def infer_entries(torch, dev):
    """(name, call, {tensor: valid rows}) of every inference entry point and X-Pool path, at the smallest shapes that reach each
    (engine constructions as in tests/test_engine_gpu.py and tests/test_shortlist_gpu.py)."""
    from mgsv_amd import synth
    from mgsv_amd.config import cfg_headline, cfg_native
    from mgsv_amd.engine import MadeEngine
    put = lambda d: {k: torch.from_numpy(v).to(dev) for k, v in d.items() if isinstance(v, np.ndarray)}

    def engine(cfg, dtype):
        return MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device=dev, dtype=dtype)

    for name, (dtype, (B, Tv, Ta), over) in CONFIGS.items():
        cfg = dataclasses.replace(cfg_headline(), **over)
        t = put(synth.make_inputs(cfg, B, Tv, Ta, seed=1))
        valid = valid_rows(cfg, t["frame_masks"], t["segment_masks"])
        for losses in (True, False):                     # (a fresh engine each: both record the first call on their workspace)
            yield (f"forward/{name}/{'losses' if losses else 'eval'}",
                   lambda e=engine(cfg, dtype), t=t, losses=losses: e.forward(t["frame_feats"], t["segment_feats"], t["frame_masks"], t["segment_masks"],
                                                                              t["spans_target"], with_losses=losses, v_duration=t["v_duration"]), valid)
    for name in ("headline", "ca"):                      # 5 pairs in batches of 4: the last batch is padded
        cfg = dataclasses.replace(cfg_headline(), **CONFIGS[name][2])
        e, t = engine(cfg, "bf16"), put(synth.make_inputs(cfg, *SMALL, seed=1))
        videos, music = e.encode_videos(t["frame_feats"], t["frame_masks"], t["v_duration"]), e.encode_music(t["segment_feats"], t["segment_masks"])
        yield (f"localize_pairs/{name}", lambda e=e, v=videos, m=music: e.localize_pairs(v, m, [0, 1, 2, 3, 1], [1, 0, 3, 2, 2], pair_batch=4), {})
    retrieval = dict(sims=(cfg_native, "bf16", (257, 5, 40), None), fused=(cfg_native, "bf16", (257, 5, 130), None),
                     attention=(cfg_headline, "bf16", (257, 5, 40), 2), wide_hoisted=(cfg_native, "f32", (8, 5, 6), 2),
                     wide=(cfg_native, "f32", (4, 5, 6), 2), inbatch=(cfg_native, "bf16", (8, 3, 256), None))
    for name, (make, dtype, (Nv, Nm, S), chunk_m) in retrieval.items():
        cfg = make()
        e, t = engine(cfg, dtype), put(synth.make_retrieval_inputs(Nv, Nm, S, cfg.D, seed=7, min_len=3))
        yield (f"retrieval_sim_matrix/{name}", lambda e=e, t=t, chunk_m=chunk_m: dict(sim=e.retrieval_sim_matrix(
            t["video_embeds"], t["segment_embeds"], t["segment_masks"], t["music_embeds"], chunk_m=chunk_m)), {})
    rng = np.random.default_rng(5)
    lists = [[], [5], list(range(33)), list(range(70)), *(np.sort(rng.choice(70, n, replace=False)).tolist() for n in (7, 40, 64)), [69], [3, 9]]
    start = torch.tensor(np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32), device=dev)
    vidx = torch.tensor(np.concatenate([np.asarray(l, np.int32) for l in lists]), device=dev)
    for dtype in ("bf16", "f32"):                        # the pair kernel; every video against the tracks + a gather
        cfg = cfg_native()
        e, t = engine(cfg, dtype), put(synth.make_retrieval_inputs(70, len(lists), 40, cfg.D, seed=7, min_len=3))
        yield (f"xpool_pair_sims/{dtype}", lambda e=e, t=t: dict(pair_sims=e.xpool_pair_sims(
            t["video_embeds"], t["segment_embeds"].to(e.tc), t["segment_masks"], start, vidx, max_count=max(len(l) for l in lists))), {})


def record_infer(a) -> None:
    torch, dev = setup(a)
    from mgsv_amd.tape import LaunchTape
    res, arrays = dict(tree=os.path.abspath(a.tree), entries={}), {}
    for name, call, valid in infer_entries(torch, dev):
        torch.cuda.synchronize()
        with torch.no_grad(), LaunchTape.record(check=False) as tape:
            out = call()
        torch.cuda.synchronize()
        e = res["entries"][name] = dict(ops=numbered(tape.ops()), foreign=list(tape.foreign_ops), out={})
        tape.close()
        for k, v in out.items():
            if isinstance(v, torch.Tensor):
                x = v.detach() if valid.get(k) is None else v.detach()[valid[k]]
                e["out"][k] = sha(x)
                arrays[f"{name}:{k}"] = (x.float() if x.is_floating_point() else x).cpu().numpy()
        print(f"{name}: {len(e['ops'])} operations, {len(e['foreign'])} framework kernels, {len(e['out'])} tensors", flush=True)
    np.savez(os.path.splitext(a.out)[0] + ".npz", **arrays)
    with open(a.out, "w") as f:
        json.dump(res, f)


def same(label: str, part: str, p, n) -> bool:
    """one list or table of hashes of two records: prints the verdict, and the differing keys of a table"""
    eq = json.dumps(p, sort_keys=True) == json.dumps(n, sort_keys=True)
    print(f"{label:10s} {part:8s} {'equal' if eq else 'DIFFERENT'}" + (f"  ({len(p)} entries)" if part != "counts" else f"  {p} = {sum(p)}"))
    if not eq and isinstance(p, dict):
        print("    differing:", [k for k in set(p) | set(n) if p.get(k) != n.get(k)])
    return eq


def compare(a) -> None:
    """Lists and hashes must be equal.  flat_grad: largest per-tensor relative L2 difference over the parent-parent pairs and over the
    new-parent pairs of runs; no tensor's new-parent figure may exceed twice the largest parent-parent figure (3h: one pair is a draw)."""
    p, n = (json.load(open(f)) for f in (a.parent, a.new))
    gp, gn = (np.load(os.path.splitext(f)[0] + ".npy") for f in (a.parent, a.new))
    ok = True
    for part in ("ops", "foreign", "counts", "forward", "backward", "params"):
        ok &= same(p["config"], part, p[part], n[part])
    names, starts = [k for k, _, _ in p["params"]], np.array([o for _, o, _ in p["params"]])      # (offsets ascend; padding holds zeros)

    def rel(x, y):                                           # per tensor ||x - y|| / ||y||, 0 where both vanish
        x, y = x.astype(np.float64), y.astype(np.float64)
        d, ny = np.sqrt(np.add.reduceat((x - y) ** 2, starts)), np.sqrt(np.add.reduceat(y ** 2, starts))
        return np.where(d == 0, 0.0, d / np.maximum(ny, 1e-300))
    pp = np.max([rel(gp[i], gp[j]) for i, j in itertools.combinations(range(len(gp)), 2)], axis=0)
    nw = np.max([rel(x, y) for x in gn for y in gp], axis=0)
    bound = 2 * pp.max()
    within = bool((nw <= bound).all())
    ok &= within
    print(f"{p['config']:10s} flat_grad parent-parent {pp.max():.4g} ({names[pp.argmax()]}), new-parent {nw.max():.4g} ({names[nw.argmax()]}): "
          f"{'within' if within else 'OUTSIDE'} 2 x parent-parent  [{len(gp)} + {len(gn)} runs]")
    sys.exit(0 if ok else 1)


def compare_infer(a) -> None:
    """Per entry `ops` and `foreign` must be equal, and every tensor's hash wherever the parent's two records agree.  A tensor the parent does
    not reproduce is named, and the new record may differ from either parent record by at most twice the parents' largest difference."""
    p, p2, n = (json.load(open(f))["entries"] for f in (a.parent, a.parent2, a.new))
    zp, zp2, zn = (np.load(os.path.splitext(f)[0] + ".npz") for f in (a.parent, a.parent2, a.new))
    ok = set(p) == set(p2) == set(n)
    tensors = loose = 0
    for name in p:
        ok &= same(name, "ops", p[name]["ops"], n[name]["ops"]) & same(name, "foreign", p[name]["foreign"], n[name]["foreign"])
        steady = {k: h for k, h in p[name]["out"].items() if p2[name]["out"].get(k) == h}
        ok &= same(name, "out", steady, {k: h for k, h in n[name]["out"].items() if k in steady or k not in p[name]["out"]})
        tensors += len(steady)
        for k in sorted(set(p[name]["out"]) - set(steady)):
            x, x2, y = (z[f"{name}:{k}"].astype(np.float64) for z in (zp, zp2, zn))
            pp, nw = np.abs(x - x2).max(), max(np.abs(y - x).max(), np.abs(y - x2).max())
            within = bool(nw <= 2 * pp)
            ok &= within
            loose += 1
            print(f"{name:10s} {k}: the parent does not reproduce it: parent-parent {pp:.4g}, new-parent {nw:.4g} (max abs): "
                  f"{'within' if within else 'OUTSIDE'} 2 x parent-parent")
    print(f"{len(p)} entries, {sum(len(e['ops']) for e in p.values())} operations, {tensors} tensors compared by hash, {loose} by value: "
          f"{'all equal' if ok else 'DIFFERENT'}")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("record")
    r.add_argument("--tree", default=HERE); r.add_argument("--config", choices=sorted(CONFIGS), required=True)
    r.add_argument("--out", required=True); r.add_argument("--runs", type=int, default=5)
    r = sub.add_parser("record-infer")
    r.add_argument("--tree", default=HERE); r.add_argument("--out", required=True)
    c = sub.add_parser("compare")
    c.add_argument("parent"); c.add_argument("new")
    c = sub.add_parser("compare-infer")
    c.add_argument("parent"); c.add_argument("parent2"); c.add_argument("new")
    a = ap.parse_args()
    {"record": record, "record-infer": record_infer, "compare": compare, "compare-infer": compare_infer}[a.cmd](a)
