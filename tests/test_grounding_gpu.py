"""GPU: grounding -- localization of arbitrary (video, track) pairs from per-item tower outputs (MadeEngine.encode_videos /
encode_music / localize_pairs) against MadeEngine.forward (bit for bit) and the f32 oracle, `ground()` end to end, the sharded
music side's packed records, the refusal of the batch-dependent query, and the driver's --ground_topk."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from mgsv_amd import ops, synth
from mgsv_amd.config import cfg_native
from oracle import made_oracle as O

pytestmark = pytest.mark.gpu

# bf16 engine against the f32 oracle: the bf16 forward bounds tests/test_engine_gpu.py states for these outputs
BF16_FORWARD_TOL = dict(pred_logits=4.5e-2, pred_spans=7e-3)


def _cfg(name):
    c = cfg_native()
    if name == "CA":
        c.mml_fusion = "CA"
    elif name == "Q3":
        c.num_moment_queries = 3
    elif name == "prenorm":
        c.detr_pre_norm = True
    elif name == "regression":
        c.mml_localization = "regression"
    elif name == "center":
        c.predict_center = 1
    return c


def _setup(name, dtype, B=8, Tv=20, Ta=40, seed=0):
    from mgsv_amd.engine import MadeEngine
    cfg = _cfg(name)
    sd = synth.make_state_dict(cfg, seed=seed)
    inp = synth.make_inputs(cfg, B, Tv, Ta, seed=seed + 1)
    t = {k: torch.from_numpy(v).cuda() for k, v in inp.items() if isinstance(v, np.ndarray)}
    return cfg, sd, inp, t, MadeEngine(cfg, sd, device="cuda:0", dtype=dtype)


def _forward(eng, t, vi=None, mi=None):
    vi = torch.arange(t["frame_feats"].shape[0]) if vi is None else torch.as_tensor(vi)
    mi = vi if mi is None else torch.as_tensor(mi)
    vi, mi = vi.cuda().long(), mi.cuda().long()
    o = eng.forward(t["frame_feats"][vi].contiguous(), t["segment_feats"][mi].contiguous(), t["frame_masks"][vi].contiguous(),
                    t["segment_masks"][mi].contiguous(), t["spans_target"][vi].contiguous(), v_duration=t["v_duration"][vi].contiguous())
    lg = o["pred_logits"].clone() if "pred_logits" in o else None
    sp = o["pred_spans"].clone()
    torch.cuda.synchronize()
    return lg, sp


def _encode(eng, t, B):
    V = eng.encode_videos(t["frame_feats"], t["frame_masks"], t["v_duration"], batch=B)
    M = eng.encode_music(t["segment_feats"], t["segment_masks"], batch=B)
    return V, M


CASES = ["concat", "CA", "Q3", "prenorm", "regression", "center"]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_identity_pairing_is_the_forward(name, dtype):
    """Pairs (b, b) of a batch encoded with batch = B and localized with pair_batch = B: bit for bit what forward gives."""
    cfg, sd, inp, t, eng = _setup(name, dtype)
    B = t["frame_feats"].shape[0]
    lg, sp = _forward(eng, t)
    V, M = _encode(eng, t, B)
    r = eng.localize_pairs(V, M, torch.arange(B), torch.arange(B), pair_batch=B)
    torch.cuda.synchronize()
    assert torch.equal(r["pred_spans"], sp), float((r["pred_spans"] - sp).abs().max())
    if lg is None:
        assert r["pred_logits"] is None
    else:
        assert torch.equal(r["pred_logits"], lg), float((r["pred_logits"] - lg).abs().max())


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", ["concat", "CA", "Q3", "regression"])
def test_arbitrary_pairing_is_the_forward_on_the_assembled_batch(name, dtype):
    """Repeated, crossed and permuted pairs: forward on frame_feats[vi], segment_feats[mi] at the same P (bit for bit), and the f32
    oracle on the same pairs (f32 within 1e-4, bf16 within the forward's bf16 bounds)."""
    cfg, sd, inp, t, eng = _setup(name, dtype)
    B = t["frame_feats"].shape[0]
    vi = [3, 3, 0, 7, 1, 5, 2, 6]
    mi = [1, 4, 4, 0, 7, 2, 6, 6]
    lg, sp = _forward(eng, t, vi, mi)
    V, M = _encode(eng, t, B)
    r = eng.localize_pairs(V, M, vi, mi, pair_batch=len(vi))
    torch.cuda.synchronize()
    assert torch.equal(r["pred_spans"], sp), float((r["pred_spans"] - sp).abs().max())
    if lg is not None:
        assert torch.equal(r["pred_logits"], lg), float((r["pred_logits"] - lg).abs().max())
    a, b = np.asarray(vi), np.asarray(mi)
    with torch.no_grad():
        ref = O.forward(O.to_torch_params(sd), cfg, inp["frame_feats"][a], inp["segment_feats"][b], inp["frame_masks"][a],
                        inp["segment_masks"][b], inp["spans_target"][a], v_duration=inp["v_duration"][a])
    for key in ("pred_logits", "pred_spans"):
        if r[key] is None:
            continue
        tol = 1e-4 if dtype == "f32" else BF16_FORWARD_TOL[key]
        err = float(np.abs(r[key].cpu().numpy() - ref[key].numpy()).max())
        assert err <= tol, (key, err)


def _oracle_moments(cfg, sd, fv, fm, vd, sf, sm, mdur, vi, mi):
    """The oracle's moment of each pair: top-scoring query's span in seconds, clamped to [0, min(max_m_duration, duration)]."""
    with torch.no_grad():
        ref = O.forward(O.to_torch_params(sd), cfg, fv[vi], sf[mi], fm[vi], sm[mi], np.zeros((len(vi), 1, 2), np.float32) + 0.5,
                        v_duration=vd[vi], with_losses=False)
    lg, sp = ref["pred_logits"].numpy(), ref["pred_spans"].numpy()
    e = np.exp(lg - lg.max(-1, keepdims=True))
    prob = (e / e.sum(-1, keepdims=True))[..., cfg.foreground_label]
    q = prob.argmax(1)
    c, w = sp[np.arange(len(vi)), q, 0], sp[np.arange(len(vi)), q, 1]
    hi = np.minimum(float(cfg.max_m_duration), mdur[mi])
    st = np.minimum(np.maximum((c - 0.5 * w) * cfg.max_m_duration, 0), hi)
    en = np.minimum(np.maximum((c + 0.5 * w) * cfg.max_m_duration, 0), hi)
    return st, en, prob[np.arange(len(vi)), q]


def _library(cfg, Nv=200, Nm=60, Tv=12, Ta=24):
    v = synth.make_inputs(cfg, Nv, Tv, Ta, seed=3)
    m = synth.make_inputs(cfg, Nm, Tv, Ta, seed=4)
    mdur = np.random.default_rng(5).uniform(20.0, 300.0, size=Nm).astype(np.float32)
    gid = np.arange(Nm) % 45                                    # 15 tracks listed twice
    return v, m, mdur, gid


def test_ground_end_to_end_f32():
    from mgsv_amd.engine import MadeEngine
    from mgsv_amd.grounding import ground, similarity_matrix
    cfg = cfg_native()
    sd = synth.make_state_dict(cfg, seed=0)
    eng = MadeEngine(cfg, sd, device="cuda:0", dtype="f32")
    v, m, mdur, gid = _library(cfg)
    c = lambda x: torch.from_numpy(x).cuda()
    V = eng.encode_videos(c(v["frame_feats"]), c(v["frame_masks"]), c(v["v_duration"]), batch=64)
    M = eng.encode_music(c(m["segment_feats"]), c(m["segment_masks"]), c(mdur), batch=64)
    k = 3
    g = ground(eng, V, M, k, group_id=gid, pair_batch=64)
    sims = similarity_matrix(eng, V.vec, M.tokens, M.mask, M.vec)
    idx, sc = ops.topk_groups(sims, k, torch.from_numpy(gid.astype(np.int32)).cuda(), 45)
    torch.cuda.synchronize()
    assert torch.equal(g.track, idx) and torch.equal(g.score, sc)
    tr = g.track.cpu().numpy()
    assert (tr >= 0).all() and all(len(set(gid[row])) == k for row in tr)      # k distinct music ids per video
    vi = np.repeat(np.arange(len(tr)), k)
    mi = tr.reshape(-1)
    st, en, pr = _oracle_moments(cfg, sd, v["frame_feats"], v["frame_masks"], v["v_duration"], m["segment_feats"], m["segment_masks"],
                                 mdur, vi, mi)
    gs, ge, gc = (x.cpu().numpy().reshape(-1) for x in (g.start, g.end, g.confidence))
    # seconds = span * max_m_duration (240): the f32 forward's span error (~5e-7 of the track) becomes ~1.1e-4 s -- measured
    # 1.07e-4 s over these 600 pairs, a few float32 ulps of a moment boundary near 200 s.  Bound: 2.5e-4 s (1e-6 of max_m_duration).
    err = max(np.abs(gs - st).max(), np.abs(ge - en).max())
    assert err <= 1e-6 * cfg.max_m_duration + 1e-5, err
    assert np.abs(gc - pr).max() <= 1e-4
    hi = np.minimum(float(cfg.max_m_duration), mdur[mi])
    assert (gs <= ge).all() and (gs >= 0).all() and (ge <= hi).all()
    recs = g.to_records([f"v{i}" for i in range(len(tr))], [f"m{j}" for j in gid])
    assert len(recs) == len(tr) and all(len(r["tracks"]) == k for r in recs)
    json.dumps(recs)


def test_ground_on_the_sharded_record_views_equals_plain_tensors():
    """The music side packed into the records the sharded retrieval's all-gather delivers (ShardedRetrieval._layout), read through
    the strided views gather_music_side returns: the same grounding as on the plain tensors."""
    from mgsv_amd.engine import Encoded, MadeEngine
    from mgsv_amd.grounding import ground
    from mgsv_amd.retrieval import ShardedRetrieval
    cfg = cfg_native()
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="bf16")
    v, m, mdur, gid = _library(cfg, Nv=96, Nm=40)
    c = lambda x: torch.from_numpy(x).cuda()
    V = eng.encode_videos(c(v["frame_feats"]), c(v["frame_masks"]), c(v["v_duration"]))
    M = eng.encode_music(c(m["segment_feats"]), c(m["segment_masks"]), c(mdur))
    Nm, S, D = M.tokens.shape
    a, b, rec = ShardedRetrieval._layout(S, D, M.tokens.element_size())
    buf = torch.empty(Nm, rec, device="cuda", dtype=torch.uint8)
    ops.pack_music_records(M.tokens, M.mask, M.vec, buf, eng.tc)
    seg = buf[:, :a].view(eng.tc).view(Nm, S, D)
    mask = buf[:, a:b].view(torch.float32).view(Nm, S)
    music = buf[:, b:b + D * 4].view(torch.float32).view(Nm, D)
    assert seg.stride(0) != S * D
    Mv = Encoded(tokens=seg, mask=mask, vec=music, duration=M.duration)
    g1 = ground(eng, V, M, 5, group_id=gid % 30)
    g2 = ground(eng, V, Mv, 5, group_id=gid % 30)
    torch.cuda.synchronize()
    for f in ("track", "score", "start", "end", "confidence"):
        assert torch.equal(getattr(g1, f), getattr(g2, f)), f


def test_xpool_query_is_refused():
    from mgsv_amd.grounding import ground
    cfg, sd, inp, t, eng = _setup("concat", "f32", B=4)
    eng.cfg.moment_query_type = "xpool"
    V, M = _encode(eng, t, 4)
    with pytest.raises(NotImplementedError, match="averaged over the videos"):
        eng.localize_pairs(V, M, [0, 1], [1, 0])
    with pytest.raises(NotImplementedError):
        ground(eng, V, M, 2)


COMMON = ["--mml_fusion", "concat", "--detr_enc_layers", "2", "--audio_short_cut", "0", "--max_v_frames", "20", "--max_m_duration", "100",
          "--synthetic_features", "1", "--num_workers", "0", "--batch_size_val", "16", "--save_model", "0", "--tb_writer", "0"]


def _csv(path, n, seed):
    """the tiny split of tests/test_driver_gpu.py"""
    rng = np.random.default_rng(seed)
    cols = "video_id,music_id,video_start,video_end,music_start,music_end,music_total_duration,video_segment_duration,music_segment_duration," \
           "music_path,video_total_duration,video_width,video_height,video_total_frames,video_frame_rate,video_category"
    with open(path, "w") as f:
        f.write(cols + "\n")
        for i in range(n):
            dur = rng.uniform(40, 100)
            vd = rng.uniform(8, 19)
            ms = rng.uniform(0, dur - vd - 1)
            f.write(f"{100000 + i},m{int(rng.integers(0, max(2, n // 2)))},0.0,{vd:.3f},{ms:.3f},{ms + vd:.3f},{dur:.3f},{vd:.3f},{vd:.3f},/x.mp3,{vd:.2f},"
                    f"720,1280,300,30,Cat\n")


def test_driver_ground_topk(tmp_path):
    from mgsv_amd import driver
    va = str(tmp_path / "val.csv")
    _csv(va, 32, 2)
    base = ["--name", "g", "--test_csv", va, "--output_dir", str(tmp_path / "logs")] + COMMON
    out = driver.main_test(base + ["--ground_topk", "5"])
    files = glob.glob(str(tmp_path / "logs" / "*" / "*+g" / "ground_test_0.json"))
    assert len(files) == 1
    recs = json.load(open(files[0]))
    assert len(recs) == 32 and all(len(r["tracks"]) == 5 for r in recs)
    assert all(set(r) == {"video_id", "music_id", "gt_moment", "tracks"} for r in recs)
    assert all(set(e) == {"music_id", "score", "start", "end", "confidence"} for r in recs for e in r["tracks"])
    gr, com = out["ground"], out["com"]
    assert set(gr) == {f"GR{k}_iou{t}" for k in (1, 5, 10) for t in (0.5, 0.7)}
    # pairs are independent: the moment in the retrieved ground-truth track is the one the batched evaluation scored, so GR1 equals
    # the composite R1 -- up to the videos whose IoU sits within 1e-5 of the threshold (float rounding of two evaluations)
    for th in (0.5, 0.7):
        near = 0
        for r in recs:
            e = r["tracks"][0]
            if e["music_id"] != r["music_id"]:
                continue
            gs, ge = r["gt_moment"]
            inter = max(min(ge, e["end"]) - max(gs, e["start"]), 0.0)
            union = (e["end"] - e["start"]) + (ge - gs) - inter
            near += abs((inter / union if union > 0 else 0.0) - th) <= 1e-5
        assert abs(gr[f"GR1_iou{th}"] - com[f"R1_iou{th}"]) * 32 / 100 <= near + 1e-6, (th, gr, com)
    # --ground_topk 0 (the default): the same metrics, no grounding key, no file
    out0 = driver.main_test(base)
    assert "ground" not in out0
    assert out0["ret"] == out["ret"] and out0["loc"] == out["loc"] and out0["com"] == out["com"] and len(out0["com"]) == 12
