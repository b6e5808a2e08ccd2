"""Fingerprint of one training step, for changes that must not move an operation of the recorded step (docs/EXPERIMENTS.md 3h, 3h-2): run it
once per (tree, configuration) on ONE build of the library and compare the files.
  python tools/step_fingerprint.py record --tree PATH --config NAME --out F.json [--runs 5]    (a fresh process, one GPU; PATH holds mgsv_amd/)
  python tools/step_fingerprint.py compare PARENT.json NEW.json                                 (no GPU; exit status 1 when something differs)
F.json: (a) `ops`: the recorded step's (kind, function, stream, grid) with functions and streams numbered by first appearance, recorded with
the tape's duplicate-dependency pass off and in program order, so that every wait the Python issues is there; `foreign`: the framework
kernels inside the step (such a step cannot be replayed: recorded with MADE_TAPE_CHECK=0); `counts`: the default tape's (launches, event
operations, others).  (b) `forward`: SHA-256 per tensor of forward_train's dictionary (seed 7), valid rows only where kernels skip padded rows.
(c) `backward`: SHA-256 of the decoder's data-gradient chain after one eager train_step (seed 7, learning rates 0); F.npy: flat_grad of `runs`
such steps (f32 atomic adds in a free order: compared as distributions, see compare())."""
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


def record(a) -> None:
    os.environ["MADE_DEBUG_VARIANTS"] = "1"                    # (measurement knobs are honoured only under this switch)
    os.environ["MADE_TAPE_CHECK"] = "0"
    os.environ.setdefault("MADE_LIB_PATH", os.path.join(HERE, "mgsv_amd", "libmade_hip.so"))   # the build is always this tree's
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from mgsv_amd import synth
    from mgsv_amd.config import cfg_headline
    from mgsv_amd.trainer import MadeTrainer
    dtype, (B, Tv, Ta), over = CONFIGS[a.config]
    cfg = dataclasses.replace(cfg_headline(), **over)
    dev = torch.device("cuda", 0)
    trn = MadeTrainer(cfg, synth.make_state_dict(cfg, seed=0), device=dev, dtype=dtype)
    t = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_inputs(cfg, B, Tv, Ta, seed=1).items() if isinstance(v, np.ndarray)}
    batch = (t["frame_feats"], t["segment_feats"], t["frame_masks"], t["segment_masks"], t["spans_target"])
    fm, sm = batch[2].bool(), batch[3].bool()

    def sha(x, valid=None) -> str:
        x = x.detach() if valid is None else x.detach()[valid]
        return hashlib.sha256(x.contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()

    # (b) padded rows of these are skipped by design and hold whatever the buffer held
    valid = dict(frame_feats=fm, proj_vid_mem=fm, segment_feats=sm, memory=torch.cat([fm, sm], 1) if "concat" in cfg.mml_fusion else sm)
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
    fns, sts = {}, {}
    res["ops"] = [(k, fns.setdefault(fn, len(fns)), sts.setdefault(st, len(sts)), grid) for k, fn, st, grid in g.tape.ops()]
    res["foreign"] = list(g.tape.foreign_ops)
    g.close()
    g = tape()
    res["counts"] = g.tape.counts()
    g.close()
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(f"{a.config} [{a.tree}]: {len(res['ops'])} operations without the dedup pass, {len(res['foreign'])} framework kernels; default tape "
          f"{res['counts']} = {sum(res['counts'])}")


def compare(a) -> None:
    """Lists and hashes must be equal.  flat_grad: largest per-tensor relative L2 difference over the parent-parent pairs and over the
    new-parent pairs of runs; no tensor's new-parent figure may exceed twice the largest parent-parent figure (3h: one pair is a draw)."""
    p, n = (json.load(open(f)) for f in (a.parent, a.new))
    gp, gn = (np.load(os.path.splitext(f)[0] + ".npy") for f in (a.parent, a.new))
    ok = True
    for part in ("ops", "foreign", "counts", "forward", "backward", "params"):
        same = json.dumps(p[part], sort_keys=True) == json.dumps(n[part], sort_keys=True)
        ok &= same
        print(f"{p['config']:10s} {part:8s} {'equal' if same else 'DIFFERENT'}" + (f"  ({len(p[part])} entries)" if part != "counts" else f"  {p[part]} = {sum(p[part])}"))
        if not same and isinstance(p[part], dict):
            print("    differing:", [k for k in set(p[part]) | set(n[part]) if p[part].get(k) != n[part].get(k)])
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("record")
    r.add_argument("--tree", default=HERE); r.add_argument("--config", choices=sorted(CONFIGS), required=True)
    r.add_argument("--out", required=True); r.add_argument("--runs", type=int, default=5)
    c = sub.add_parser("compare")
    c.add_argument("parent"); c.add_argument("new")
    a = ap.parse_args()
    record(a) if a.cmd == "record" else compare(a)
