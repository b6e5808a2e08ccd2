"""GPU parity of the full hot path (MadeEngine: every kernel through the C ABI) against the CPU
oracle and the reference's golden vectors.

f32 engine: <= 1e-4 on logits / spans / features / similarities (north_star), matcher indices
identical.  bf16 engine (bf16 MFMA, f32 accumulate, bf16 activations in HBM): stated tolerance
5e-2 on logits/spans, 5e-3 on retrieval similarities (the reference's own CPU bf16 autocast moves pred_logits
by 6e-3 at one layer depth; here every activation between kernels is bf16)."""
import ast
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mgsv_amd import synth  # noqa: E402
from mgsv_amd.config import cfg_headline, cfg_native, cfg_plumbing  # noqa: E402
from mgsv_amd.engine import MadeEngine  # noqa: E402
from oracle import made_oracle as O  # noqa: E402

SUB = (slice(None), slice(None, None, 7), slice(None, None, 5))
# bf16 retrieval similarities against the f32 oracle: 2x the largest error measured over every shape and kernel of this file
# (tools/retrieval_parity_probe.py -> profiles/r05_retrieval_parity_probe.txt: D = 256 <= 2.5e-3 up to 53 000 x 4 000, D = 512 <= 1.1e-3).
# The cosine similarities are divided by tau = 0.03 downstream (model_Uni.py:29), so 5e-3 is a sixth of one logit.
BF16_SIM_TOL = 5e-3
BF16_SIM_TOL_D512 = 2.5e-3


def _oracle(cfg, sd, inp):
    with torch.no_grad():
        return O.forward(O.to_torch_params(sd), cfg, inp["frame_feats"], inp["segment_feats"], inp["frame_masks"],
                         inp["segment_masks"], inp["spans_target"], v_duration=inp["v_duration"])


# bf16 engine against the f32 oracle: 2x the largest error measured over the 15 shapes of tools/bf16_error_probe.py (profiles/r05_bf16_error_probe.txt:
# clip vectors 1.1e-3, dual similarities 1.1e-3, in-batch single similarities 8.9e-4, logits 2.2e-2, spans 3.4e-3, losses 9.2e-3 relative).
# Rounds 1-4 allowed 5e-3 / 1e-2 / 3e-2 / 5e-2 / 2e-2 / 5e-2.
BF16_FORWARD_TOL = dict(video_feats=2.5e-3, music_feats=2.5e-3, sims_dual=2.5e-3, sims_single=2e-3, pred_logits=4.5e-2, pred_spans=7e-3)
BF16_LOSS_RTOL = 2e-2


def _cases():
    c3 = cfg_native(); c3.num_moment_queries = 3
    c4 = cfg_native(); c4.fb_label = "10"; c4.with_act_after_proj = 1; c4.vmr_loss = "dual_single_sim_fuse"
    c5 = cfg_native(); c5.moment_query_type = "music"; c5.contrastive_align_loss = 0; c5.vmr_loss = "single"
    c6 = cfg_native(); c6.mml_fusion = "CA"
    c7 = cfg_native(); c7.fusion_mask = 0; c7.moment_query_type = "zero"; c7.aux_loss = 1
    c8 = cfg_native(); c8.dim_input = 128; c8.SA_temporal_heads = 4; c8.detr_nheads = 4    # a narrow model (32-wide heads): the slow-but-correct widths
    c9 = cfg_native(); c9.detr_pre_norm = True                  # pre-norm DETR layers (reference music_detr/transformer.py:170-189,246-271)
    c10 = cfg_headline(); c10.detr_pre_norm = True; c10.num_moment_queries = 2
    return {
        "pre_norm_B5": (c9, 5, 50, 96),
        "pre_norm_Q2_cfg2_shape_B3": (c10, 3, 30, 512),
        "narrow_D128_B4": (c8, 4, 50, 96),
        "native_CA_fusion_B4": (c6, 4, 50, 96),
        "native_nomask_zeroquery_B4": (c7, 4, 50, 96),
        "cfg1_B2": (cfg_plumbing(), 2, 30, 200),
        "native_B8": (cfg_native(), 8, 50, 96),
        "native_Q3_B4": (c3, 4, 50, 96),
        "native_fb10_act_simfuse_B5": (c4, 5, 50, 96),
        "native_musicquery_nocontrast_B3": (c5, 3, 50, 96),
        "cfg2_shape_B4": (cfg_headline(), 4, 30, 512),
        "ragged_B3_Tv7_Ta13": (cfg_native(), 3, 7, 13),
        "single_sample_B1_Tv3_Ta5": (cfg_native(), 1, 3, 5),
        "odd_B7_Tv33_Ta131": (cfg_native(), 7, 33, 131),
    }


@pytest.mark.parametrize("dtype", ["f32", "f32x3"])
@pytest.mark.parametrize("name", list(_cases()))
def test_f32_forward_matches_oracle(name, dtype):
    """dtype "f32": exact-f32 MFMA.  "f32x3" (round 6): the same f32 engine with every matrix product as three bf16 products on split operands
    (f32_products = 1 in each launch's arguments, csrc/common.h) -- held to the SAME 1e-4 gate on every output."""
    cfg, B, Tv, Ta = _cases()[name]
    sd = synth.make_state_dict(cfg, seed=0)
    inp = synth.make_inputs(cfg, B, Tv, Ta, seed=1, min_len_v=min(5, Tv), min_len_a=min(12, Ta))
    eng = MadeEngine(cfg, sd, dtype=dtype)
    out = eng.forward_numpy(inp)
    ref = _oracle(cfg, sd, inp)
    tol = 1e-4
    for k in ("video_feats", "music_feats", "frame_feats", "segment_feats", "sims_single", "sims_dual",
              "pred_logits", "pred_spans"):
        np.testing.assert_allclose(out[k], ref[k].numpy(), atol=tol, rtol=0, err_msg=k)
    # the encoder memory is only defined (and only ever read) at valid tokens: padded tokens are skipped on the HIP path
    fmask = np.concatenate([inp["frame_masks"], inp["segment_masks"]], 1) if "concat" in cfg.mml_fusion else inp["segment_masks"]
    valid = fmask != 0
    np.testing.assert_allclose(out["memory"][valid], ref["memory"].numpy()[valid], atol=tol, rtol=0, err_msg="memory")
    np.testing.assert_allclose(out["music_feats_pooled"], ref["music_feats_pooled"].numpy(), atol=tol, rtol=0)
    np.testing.assert_allclose(out["hs"], ref["hs"].numpy(), atol=tol, rtol=0)
    nd = cfg.detr_dec_layers
    for i, aux in enumerate(ref["aux_outputs"]):
        np.testing.assert_allclose(out["logits_all"][i], aux["pred_logits"].numpy(), atol=tol, rtol=0)
        np.testing.assert_allclose(out["spans_all"][i], aux["pred_spans"].numpy(), atol=tol, rtol=0)
    if cfg.contrastive_align_loss:
        np.testing.assert_allclose(out["proj_queries"], ref["proj_queries"].numpy(), atol=tol, rtol=0)
        np.testing.assert_allclose(out["proj_vid_mem"], ref["proj_vid_mem"].numpy(), atol=tol, rtol=0)
    got = [(i.tolist(), j.tolist()) for i, j in out["matcher_indices"]]
    want = [(i.tolist(), j.tolist()) for i, j in ref["matcher_indices"]]
    assert got == want
    assert set(out["loss_dict"]) == set(ref["loss_dict"])
    for k, v in ref["loss_dict"].items():
        np.testing.assert_allclose(out["loss_dict"][k], float(v), rtol=2e-4, atol=2e-4, err_msg=k)
    np.testing.assert_allclose(out["retrieval_loss"], float(ref["retrieval_loss"]), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(out["localization_loss"], float(ref["localization_loss"]), rtol=2e-4, atol=5e-4)


@pytest.mark.parametrize("dtype", ["f32", "f32x3"])
@pytest.mark.parametrize("name", ["forward_cfg1_B2", "forward_native_Q3_B4"])
def test_f32_forward_matches_reference_golden(golden_dir, name, dtype):
    """Straight against what the reference itself produced (tests/golden/make_golden.py)."""
    fix = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = cfg_plumbing() if "cfg1" in name else cfg_native()
    for k, v in ast.literal_eval(str(fix["meta_cfg_overrides"])):
        setattr(cfg, k, v)
    B, Tv, Ta = int(fix["meta_B"]), int(fix["meta_T_v"]), int(fix["meta_T_a"])
    sd = synth.make_state_dict(cfg, seed=int(fix["meta_weight_seed"]))
    inp = synth.make_inputs(cfg, B, Tv, Ta, seed=int(fix["meta_data_seed"]))
    out = MadeEngine(cfg, sd, dtype=dtype).forward_numpy(inp)
    tol = 1e-4
    for k in ("pred_logits", "pred_spans", "proj_queries", "video_feats", "music_feats", "sims_single", "sims_dual"):
        np.testing.assert_allclose(out[k], fix[k], atol=tol, rtol=0, err_msg=k)
    np.testing.assert_allclose(out["frame_feats"][SUB], fix["frame_feats_sub"], atol=tol, rtol=0)
    np.testing.assert_allclose(out["segment_feats"][SUB], fix["segment_feats_sub"], atol=tol, rtol=0)
    np.testing.assert_allclose(out["music_feats_pooled"][:, :, ::5], fix["music_feats_pooled_sub"], atol=tol, rtol=0)
    np.testing.assert_allclose(out["proj_vid_mem"][SUB], fix["proj_vid_mem"], atol=tol, rtol=0)
    nd = cfg.detr_dec_layers
    for i in range(nd - 1):
        np.testing.assert_allclose(out["logits_all"][i], fix[f"aux{i}_pred_logits"], atol=tol, rtol=0)
        np.testing.assert_allclose(out["spans_all"][i], fix[f"aux{i}_pred_spans"], atol=tol, rtol=0)
    for b, (i, j) in enumerate(out["matcher_indices"]):
        assert i.tolist() == fix["matcher_pred_idx"][b].tolist() and j.tolist() == fix["matcher_tgt_idx"][b].tolist()
    for k in [k for k in fix.files if k.startswith("loss_")]:
        np.testing.assert_allclose(out["loss_dict"][k[5:]], float(fix[k]), rtol=2e-4, atol=2e-4, err_msg=k)
    np.testing.assert_allclose(out["retrieval_loss"], float(fix["retrieval_loss"]), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(out["localization_loss"], float(fix["localization_loss"]), rtol=2e-4, atol=5e-4)


def test_fused_decoder_chain_matches_split_k_chain():
    """bf16, Q = 1: the fused decoder chain (made_dec_stage: LayerNorms in the consumers' prologues, unfolded value path) against
    round 1's split-K + finish chain on the same weights and batch: the decoder states of all layers agree to bf16 rounding."""
    for cfg, B, Tv, Ta in ((cfg_headline(), 8, 30, 512), (cfg_native(), 5, 50, 96)):
        sd = synth.make_state_dict(cfg, seed=0)
        inp = synth.make_inputs(cfg, B, Tv, Ta, seed=3)
        fused = MadeEngine(cfg, sd, dtype="bf16")
        plain = MadeEngine(cfg, sd, dtype="bf16")
        plain.force_unfused_decoder = True
        assert fused._fused_decoder() and not plain._fused_decoder()
        a, b = fused.forward_numpy(inp), plain.forward_numpy(inp)
        for k, tol in (("hs", 3e-2), ("pred_logits", 3e-2), ("pred_spans", 1e-2)):       # + 2 bf16 ulps of the value (hs reaches |8|)
            err = (np.abs(a[k] - b[k]) - 2.0 ** -7 * np.abs(b[k])).max()
            assert err <= tol, (k, float(err))
        np.testing.assert_allclose(a["localization_loss"], b["localization_loss"], rtol=2e-2)


def test_bf16_graph_replay_full_batch_properties():
    """The configuration bench.py times (B = 64, T_v = 30, T_a = 512, D = 512, bf16, hipGraph): outputs finite, the matcher accepts
    the costs, and a graph replay is bit-identical to the eager step (no launch depends on host state or on timing)."""
    cfg = cfg_headline()
    B, Tv, Ta = 64, 30, 512
    sd = synth.make_state_dict(cfg, seed=0)
    inp = synth.make_inputs(cfg, B, Tv, Ta, seed=1)
    dev = torch.device("cuda")
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items() if isinstance(v, np.ndarray)}
    eng = MadeEngine(cfg, sd, device=dev, dtype="bf16")
    step = lambda: eng.forward(t["frame_feats"], t["segment_feats"], t["frame_masks"], t["segment_masks"], t["spans_target"])
    keys = ["pred_logits", "pred_spans", "sims_single", "sims_dual", "retrieval_loss", "localization_loss", "criterion_losses", "hs",
            "matcher_pred_idx", "video_feats", "music_feats", "memory"]
    valid = torch.cat([t["frame_masks"], t["segment_masks"]], dim=1) != 0          # padded tokens of `memory` are never computed or written
    pick = lambda k, x: x[valid] if k == "memory" else x
    o = step(); torch.cuda.synchronize()
    eager = {k: pick(k, o[k]).clone() for k in keys}
    assert int(o["matcher_status"].cpu()) == 0
    for k in keys:
        assert bool(torch.isfinite(eager[k].float()).all()), k
    assert float(eager["pred_spans"].min()) >= 0.0 and float(eager["pred_spans"].max()) <= 1.0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        og = step()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(pick(k, og[k]), eager[k]), f"{k}: graph replay differs from the eager step"


@pytest.mark.parametrize("name", ["native_B8", "cfg2_shape_B4", "native_nomask_zeroquery_B4", "native_musicquery_nocontrast_B3", "single_sample_B1_Tv3_Ta5",
                                  "pre_norm_B5", "pre_norm_Q2_cfg2_shape_B3"])
def test_bf16_forward_within_stated_tolerance(name):
    cfg, B, Tv, Ta = _cases()[name]
    sd = synth.make_state_dict(cfg, seed=0)
    inp = synth.make_inputs(cfg, B, Tv, Ta, seed=1)
    out = MadeEngine(cfg, sd, dtype="bf16").forward_numpy(inp)
    ref = _oracle(cfg, sd, inp)
    for k, tol in BF16_FORWARD_TOL.items():
        err = np.abs(out[k] - ref[k].numpy()).max()
        assert err <= tol, (k, float(err))
    assert np.isfinite(out["localization_loss"]) and np.isfinite(out["retrieval_loss"])
    np.testing.assert_allclose(out["localization_loss"], float(ref["localization_loss"]), rtol=BF16_LOSS_RTOL)
    np.testing.assert_allclose(out["retrieval_loss"], float(ref["retrieval_loss"]), rtol=BF16_LOSS_RTOL, atol=BF16_LOSS_RTOL)


def test_widths_the_wide_attention_kernel_is_not_built_for_fail_at_construction():
    """--dim_input is a free flag, but made_attention_wide (X-Pool, memory-space decoder attention) is built for D = 128 / 256 / 512: any
    other width raises when the engine is constructed, in either dtype -- never inside a launch (so made_dec_stage's own 256 / 512
    limit, which _fused_decoder also checks, cannot be reached with an unsupported width).  D = 128 runs (test_f32_forward_matches_oracle
    [narrow_D128_B4], test_bf16_narrow_model_matches_oracle): the register-staged wide attention and the unfused decoder chain."""
    for D in (384, 768):
        cfg = cfg_native()
        cfg.dim_input = D
        for dtype in ("bf16", "f32"):
            with pytest.raises(NotImplementedError, match="dim_input"):
                MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), dtype=dtype)


def test_bf16_narrow_model_matches_oracle():
    """dim_input = 128 (heads of 32) in bf16: the path without the D = 256 / 512 specialisations (fused decoder stages, LDS-DMA wide attention,
    made_xpool_inbatch): forward within the bf16 tolerance of the f32 oracle."""
    cfg = cfg_native(); cfg.dim_input = 128; cfg.SA_temporal_heads = 4; cfg.detr_nheads = 4
    sd = synth.make_state_dict(cfg, seed=0)
    inp = synth.make_inputs(cfg, 6, 50, 96, seed=1)
    out = MadeEngine(cfg, sd, dtype="bf16").forward_numpy(inp)
    ref = _oracle(cfg, sd, inp)
    for k, tol in BF16_FORWARD_TOL.items():
        np.testing.assert_allclose(out[k], ref[k].numpy(), atol=tol, rtol=0, err_msg=k)
    assert np.isfinite(out["retrieval_loss"]) and abs(out["retrieval_loss"] - float(ref["retrieval_loss"])) <= BF16_LOSS_RTOL * max(1.0, abs(float(ref["retrieval_loss"])))


def test_retrieval_matches_reference_golden_and_oracle(golden_dir):
    fix = np.load(os.path.join(golden_dir, "retrieval.npz"))
    cfg = cfg_native()
    sd = synth.make_state_dict(cfg, seed=0)
    eng = MadeEngine(cfg, sd, dtype="f32")
    dev = eng.device
    for tag in ("a", "b"):
        N_v, N_m, S, D = [int(x) for x in fix[f"{tag}_shape"]]
        ri = synth.make_retrieval_inputs(N_v, N_m, S, D, seed=2)
        t = {k: torch.from_numpy(v).to(dev) for k, v in ri.items()}
        for chunk in (None, 7):            # chunking over tracks must not change a single value
            sim = eng.retrieval_sim_matrix(t["video_embeds"], t["segment_embeds"], t["segment_masks"], t["music_embeds"], chunk_m=chunk)
            torch.cuda.synchronize()
            np.testing.assert_allclose(sim.cpu().numpy(), fix[f"{tag}_sim"], atol=1e-4, rtol=0)
            if chunk is None:
                base = sim.clone()
            else:
                assert torch.equal(sim, base)
    # hoisted (Nv > S) and un-hoisted (Nv <= S) variants agree with the oracle on a fresh shape
    ri = synth.make_retrieval_inputs(40, 9, 96, cfg.D, seed=5)
    t = {k: torch.from_numpy(v).to(dev) for k, v in ri.items()}
    sim = eng.retrieval_sim_matrix(t["video_embeds"], t["segment_embeds"], t["segment_masks"], t["music_embeds"])
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = O.retrieval_sim_matrix(O.to_torch_params(sd), cfg, ri["video_embeds"], ri["segment_embeds"], ri["segment_masks"], ri["music_embeds"])
    np.testing.assert_allclose(sim.cpu().numpy(), ref.numpy(), atol=1e-4, rtol=0)


@pytest.mark.parametrize("name", ["xa_music_video_single", "xa_video_single", "predict_center", "audio_short_cut_fb10", "audio_short_cut_Q3", "xpool_query", "moment_embedding", "feature_fuse", "regression",
                                  "regression_center_CA", "shared_temporal_block", "cls_token", "agg_mlp", "pre_norm", "pre_norm_Q3_CA"])
def test_option_variants_match_reference_fixture_and_oracle(golden_dir, name):
    """the second X-Pool tower, predict_center, audio_short_cut and the regression head, f32 engine
    against the reference's own outputs (tests/golden/variants.npz) and, for the similarities, the oracle."""
    from test_oracle_golden import variant_case, check_variant
    fix = np.load(os.path.join(golden_dir, "variants.npz"))
    cfg, sd, inp = variant_case(fix, name)
    out = MadeEngine(cfg, sd, dtype="f32").forward_numpy(inp)
    check_variant(fix, name, out)
    ref = _oracle(cfg, sd, inp)
    for k in ("video_feats", "music_feats", "sims_dual", "sims_video_pooling"):
        if k in ref and k in out:
            np.testing.assert_allclose(out[k], ref[k].numpy(), atol=1e-4, rtol=0, err_msg=k)
    if "regression" in name:       # the regression head reads the encoder memory at EVERY position, padded ones included
        np.testing.assert_allclose(out["memory"], ref["memory"].numpy(), atol=1e-4, rtol=0)


def test_engine_rejects_unsupported_configs_loudly():
    cfg = cfg_native(); cfg.vmr_fusion = "XA-video"; cfg.vmr_loss = "dual_single_loss_fuse"     # the reference fails there too
    with pytest.raises(NotImplementedError):
        MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), dtype="f32")
    cfg = cfg_headline(); cfg.audio_attention_seqlen = 300
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), dtype="f32")
    inp = synth.make_inputs(cfg, 2, 30, 512, seed=1)
    with pytest.raises(ValueError):      # the reference raises at model_Base.py:533 when T_a > 300
        eng.forward_numpy(inp)


def test_retrieval_parity_across_track_chunks_at_scale():
    """Retrieval launch of the timed kind at a size where the fused kernel walks SEVERAL track chunks per video tile and more tracks
    than one chunk table holds (N_m = 2 304 > PMAX_TRACKS = 1 024; 4 352 videos = 68 video tiles): every pair is independent, so the
    f32 oracle (chunked over videos, as test-MaDe.py's matrix would be) is evaluated on all videos x a spread of track columns --
    the first / last tracks, both sides of every 1 024 boundary -- and on a stripe of video rows x ALL tracks."""
    cfg = cfg_native()
    sd = synth.make_state_dict(cfg, seed=0)
    eng = MadeEngine(cfg, sd, dtype="bf16")
    dev = eng.device
    N_v, N_m, S = 4352, 2304, 96
    ri = synth.make_retrieval_inputs(N_v, N_m, S, cfg.D, seed=11, min_len=3)
    t = {k: torch.from_numpy(v).to(dev) for k, v in ri.items()}
    sim = eng.retrieval_sim_matrix(t["video_embeds"], t["segment_embeds"], t["segment_masks"], t["music_embeds"])
    torch.cuda.synchronize()
    sim = sim.cpu()
    assert sim.shape == (N_v, N_m) and bool(torch.isfinite(sim).all())
    P = O.to_torch_params(sd)
    cols = sorted(set(list(range(0, 6)) + list(range(1018, 1030)) + list(range(2042, 2054)) + list(range(N_m - 6, N_m)) + list(range(7, N_m, 331))))
    with torch.no_grad():
        ref_c = O.retrieval_sim_matrix(P, cfg, ri["video_embeds"], ri["segment_embeds"][cols], ri["segment_masks"][cols], ri["music_embeds"][cols])
        rows = list(range(0, 8)) + list(range(2170, 2182)) + list(range(N_v - 8, N_v))
        ref_r = O.retrieval_sim_matrix(P, cfg, ri["video_embeds"][rows], ri["segment_embeds"], ri["segment_masks"], ri["music_embeds"])
    err_c = float((sim[:, cols] - ref_c).abs().max())
    err_r = float((sim[rows] - ref_r).abs().max())
    # measured (profiles/r05_retrieval_parity_probe.txt): 1.8e-3 on the columns, 2.3e-3 on the rows; the bound is 2x that, a sixth of
    # one logit at the model's temperature (tau = 0.03, model_Uni.py:29) where rounds 1-4 allowed a whole one (3e-2)
    assert err_c <= BF16_SIM_TOL and err_r <= BF16_SIM_TOL, (err_c, err_r)
    # the ranking the metric reads: per video, the oracle's best track among the checked columns is (near-)best here too
    top_ref = ref_c.argmax(dim=1)
    got_c = sim[:, cols]
    gap = got_c.max(dim=1).values - got_c.gather(1, top_ref[:, None])[:, 0]
    assert float(gap.max()) <= 2 * BF16_SIM_TOL


@pytest.mark.parametrize("sims_kernel", [False, True])
@pytest.mark.parametrize("N_v,N_m,S", [(300, 37, 96), (257, 5, 40), (640, 12, 130)])
def test_retrieval_bf16_fused_xpool_kernel(N_v, N_m, S, sims_kernel, monkeypatch):
    """made_xpool_fused (bf16, D = 256, retrieval scale): the one-kernel per-pair chain against the f32 oracle within the bf16
    tolerance of the similarity matrix, and against the unfused bf16 path (same tolerance class, different rounding points).
    sims_kernel: the same through made_xpool_sims (MADE_XPOOL_SIMS=1: the per-pair Linear as a second P.V product on u'' = W'' u)."""
    monkeypatch.setenv("MADE_XPOOL_SIMS", "1" if sims_kernel else "0")
    cfg = cfg_native()
    sd = synth.make_state_dict(cfg, seed=0)
    eng = MadeEngine(cfg, sd, dtype="bf16")
    dev = eng.device
    ri = synth.make_retrieval_inputs(N_v, N_m, S, cfg.D, seed=7, min_len=3)
    t = {k: torch.from_numpy(v).to(dev) for k, v in ri.items()}
    sim = eng.retrieval_sim_matrix(t["video_embeds"], t["segment_embeds"], t["segment_masks"], t["music_embeds"])
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = O.retrieval_sim_matrix(O.to_torch_params(sd), cfg, ri["video_embeds"], ri["segment_embeds"], ri["segment_masks"], ri["music_embeds"])
    err = float((sim.cpu() - ref).abs().max())
    assert err <= BF16_SIM_TOL, err                  # measured 1.3e-3 ... 1.7e-3 over these shapes and both kernels
    # the unfused path (taken below 256 videos): same quantity, rows computed in two slices
    parts = [eng.retrieval_sim_matrix(t["video_embeds"][a:a + 200], t["segment_embeds"], t["segment_masks"], t["music_embeds"])
             for a in range(0, N_v, 200)]
    unfused = torch.cat(parts, 0)
    torch.cuda.synchronize()
    assert float((unfused.cpu() - ref).abs().max()) <= BF16_SIM_TOL
    assert float((sim - unfused).abs().max()) <= 2 * BF16_SIM_TOL
    # ranking agreement with the oracle on the top-1 track of each video, where the margin is not a rounding tie
    top_ref = ref.topk(2, dim=1)
    clear = (top_ref.values[:, 0] - top_ref.values[:, 1]) > 2 * BF16_SIM_TOL
    assert bool((sim.cpu().argmax(1)[clear] == top_ref.indices[:, 0][clear]).all())


@pytest.mark.parametrize("N_v,N_m,S", [(300, 9, 200), (257, 5, 40), (512, 6, 512)])
def test_retrieval_bf16_two_pass_xpool_attention_at_the_headline_width(N_v, N_m, S):
    """Retrieval at D = 512 (BASELINE configs[1] / [2]'s width; reference test-MaDe.py:386-403 with modules/transformer.py:156-180): the
    attention of every (video, track) pair in made_xpool_attention (two passes per track, probabilities in LDS, LayerNorm2's
    normalisation in the tail), the folded Linear and LayerNorm3 + cosine behind it -- against the f32 oracle within the bf16 tolerance
    of the similarity matrix, and against the separate-launch bf16 chain (taken below 256 videos)."""
    cfg = cfg_headline()
    assert cfg.D == 512
    sd = synth.make_state_dict(cfg, seed=0)
    eng = MadeEngine(cfg, sd, dtype="bf16")
    dev = eng.device
    ri = synth.make_retrieval_inputs(N_v, N_m, S, cfg.D, seed=7, min_len=3)
    t = {k: torch.from_numpy(v).to(dev) for k, v in ri.items()}
    sim = eng.retrieval_sim_matrix(t["video_embeds"], t["segment_embeds"], t["segment_masks"], t["music_embeds"])
    sim2 = eng.retrieval_sim_matrix(t["video_embeds"], t["segment_embeds"], t["segment_masks"], t["music_embeds"], chunk_m=2)
    torch.cuda.synchronize()
    assert torch.equal(sim, sim2)                                       # every pair is independent of the chunking of the tracks
    with torch.no_grad():
        ref = O.retrieval_sim_matrix(O.to_torch_params(sd), cfg, ri["video_embeds"], ri["segment_embeds"], ri["segment_masks"], ri["music_embeds"])
    err = float((sim.cpu() - ref).abs().max())
    assert err <= BF16_SIM_TOL_D512, err             # measured 0.9e-3 ... 1.1e-3
    parts = [eng.retrieval_sim_matrix(t["video_embeds"][a:a + 200], t["segment_embeds"], t["segment_masks"], t["music_embeds"])
             for a in range(0, N_v, 200)]
    unfused = torch.cat(parts, 0)
    torch.cuda.synchronize()
    assert float((unfused.cpu() - ref).abs().max()) <= BF16_SIM_TOL_D512
    assert float((sim - unfused).abs().max()) <= 2 * BF16_SIM_TOL_D512
    top_ref = ref.topk(2, dim=1)
    clear = (top_ref.values[:, 0] - top_ref.values[:, 1]) > 2 * BF16_SIM_TOL_D512
    assert bool((sim.cpu().argmax(1)[clear] == top_ref.indices[:, 0][clear]).all())


@pytest.mark.parametrize("hard", [False, True])
def test_retrieval_bf16_rank_agreement_with_the_oracle(hard):
    """What the metric reads (reference test-MaDe.py:392-403 -> utils/util_test.py:32-96): R@1 / R@10 / MedianR of the bf16 HIP similarity
    matrix against the f32 oracle's on the same 1 024-sample split, both through made_recall_ranks.  hard: tracks 2k and 2k + 1 are
    near-duplicates, so EVERY row has two candidates closer than 1e-2 (median margin 1.2e-4) -- bf16 may order such a pair the other
    way (R@1 moves by the pairs it flips), but whether the ground truth is inside the top 10 must agree for >= 99.5 % of the videos.
    Measured (profiles/r05_retrieval_parity_probe.txt): easy 99.9 % / 100 % agreement on R@1 / R@10 membership, hard 85.9 % / 99.8 %;
    R@10 and MedianR identical on both sets, R@1 40.23 against 40.33 (easy), 23.54 against 24.51 (hard)."""
    from mgsv_amd.utils.util_test import Recall_metrics
    cfg = cfg_native()
    sd = synth.make_state_dict(cfg, seed=0)
    eng = MadeEngine(cfg, sd, dtype="bf16")
    ri = synth.make_ranked_retrieval_inputs(1024, 96, cfg.D, seed=22 if hard else 21, hard=hard)
    t = {k: torch.from_numpy(v).to(eng.device) for k, v in ri.items()}
    sim = eng.retrieval_sim_matrix(t["video_embeds"], t["segment_embeds"], t["segment_masks"], t["music_embeds"])
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = O.retrieval_sim_matrix(O.to_torch_params(sd), cfg, ri["video_embeds"], ri["segment_embeds"], ri["segment_masks"], ri["music_embeds"])
    assert float((sim.cpu() - ref).abs().max()) <= BF16_SIM_TOL
    srt = np.sort(ref.numpy(), axis=1)[:, ::-1]
    if hard:
        assert float(np.mean(srt[:, 0] - srt[:, 1] < 1e-2)) >= 0.99          # the set is what it claims to be
    m_h, ind_h, _ = Recall_metrics(sim)
    m_o, ind_o, _ = Recall_metrics(ref.numpy())
    assert ind_o.tolist() == O.recall_ranks_plain(ref.numpy()).tolist()      # the device ranks of the oracle's matrix are the oracle's ranks
    assert np.mean((ind_h < 10) == (ind_o < 10)) >= 0.995
    assert abs(m_h["R10"] - m_o["R10"]) <= 0.2 and abs(float(m_h["MedianR"]) - float(m_o["MedianR"])) <= 0.5
    assert int(np.abs(ind_h - ind_o).max()) <= 10                            # (measured: 5) no video's rank moves by more than a few places
    if not hard:
        assert np.mean((ind_h < 1) == (ind_o < 1)) >= 0.995 and abs(m_h["R1"] - m_o["R1"]) <= 0.3
    else:
        assert abs(m_h["R1"] - m_o["R1"]) <= 3.0                              # near-duplicate pairs flip: measured 0.98 points


def test_retrieval_parity_sampled_at_the_timed_size():
    """BASELINE configs[3]'s full size, 53 000 videos x 4 000 tracks (S = 96, D = 256): the bf16 similarity matrix of the timed launch
    against the f32 oracle on 24 video rows x ALL tracks and ALL videos x 24 track columns (spread over the whole range, so every
    video tile, every track chunk and both ends are sampled); then the f32 parity mode on the same inputs, held to north_star's 1e-4.
    Measured: bf16 2.2e-3 / 2.4e-3 (rows / columns), f32 2.5e-7 / 3.1e-7 in 815 ms per pass."""
    cfg = cfg_native()
    sd = synth.make_state_dict(cfg, seed=0)
    P = O.to_torch_params(sd)
    N_v, N_m, S = 53000, 4000, 96
    ri = synth.make_retrieval_inputs(N_v, N_m, S, cfg.D, seed=31, min_len=12)
    rows = sorted(set(np.linspace(0, N_v - 1, 24).astype(int).tolist()))
    cols = sorted(set(np.linspace(0, N_m - 1, 24).astype(int).tolist()))
    with torch.no_grad():
        ref_r = O.retrieval_sim_matrix(P, cfg, ri["video_embeds"][rows], ri["segment_embeds"], ri["segment_masks"], ri["music_embeds"])
        ref_c = O.retrieval_sim_matrix(P, cfg, ri["video_embeds"], ri["segment_embeds"][cols], ri["segment_masks"][cols], ri["music_embeds"][cols])
    for dtype, tol in (("bf16", BF16_SIM_TOL), ("f32", 1e-4), ("f32x3", 1e-4)):
        eng = MadeEngine(cfg, sd, dtype=dtype)
        t = {k: torch.from_numpy(v).to(eng.device) for k, v in ri.items()}
        sim = eng.retrieval_sim_matrix(t["video_embeds"], t["segment_embeds"], t["segment_masks"], t["music_embeds"])
        torch.cuda.synchronize()
        assert sim.shape == (N_v, N_m)
        sim_r, sim_c = sim[rows].cpu(), sim[:, cols].cpu()
        assert bool(torch.isfinite(sim).all())
        err_r, err_c = float((sim_r - ref_r).abs().max()), float((sim_c - ref_c).abs().max())
        assert err_r <= tol and err_c <= tol, (dtype, err_r, err_c)
        del eng, t, sim
        torch.cuda.empty_cache()


def test_two_batches_in_flight_match_one_at_a_time():
    """bench.py --in-flight 2: two engines (own workspace, stream, captured graph) run different batches concurrently.  Every
    output of either lane must be bit-identical to the same engine running its batch alone, replay after replay: nothing in the
    library or the workspaces may be shared between lanes, and no kernel may depend on what else is resident on the chip (round 3: the
    LDS-DMA ring GEMM kernel did -- garbage rows in ~0.5 % of such replays at the headline size; tools/race_probe_eval.py is the long
    version of this test)."""
    cfg = cfg_headline()
    B, Tv, Ta = 64, 30, 512
    sd = synth.make_state_dict(cfg, seed=0)
    dev = torch.device("cuda")
    lanes = []
    for l in range(2):
        inp = synth.make_inputs(cfg, B, Tv, Ta, seed=11 + 7 * l)
        t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items() if isinstance(v, np.ndarray)}
        lanes.append((MadeEngine(cfg, sd, device=dev, dtype="bf16"), t))

    def step(l):
        eng, t = lanes[l]
        return eng.forward(t["frame_feats"], t["segment_feats"], t["frame_masks"], t["segment_masks"], t["spans_target"])

    keys = ["pred_logits", "pred_spans", "sims_single", "sims_dual", "retrieval_loss", "localization_loss", "criterion_losses",
            "matcher_pred_idx", "video_feats", "music_feats"]
    alone = []
    for l in range(2):
        o = step(l)
        torch.cuda.synchronize()
        alone.append({k: o[k].clone() for k in keys})
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    graphs, outs = [], [None, None]
    for l in range(2):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs[l] = step(l)
        graphs.append(g)
    for it in range(300):                                # interleaved replays, both graphs in flight at once
        for l in range(2):
            with torch.cuda.stream(streams[l]):
                graphs[l].replay()
        torch.cuda.synchronize()
        for l in range(2):
            for k in keys:
                assert torch.equal(outs[l][k], alone[l][k]), f"replay {it}, lane {l}: {k} differs when two batches are in flight"


def test_f32x3_engine_leaves_the_exact_product_mode_behind():
    """The f32 product mode is an argument of each launch (f32_products), never a state of the library: an "f32x3" engine runs every f32 product
    of its own as three bf16 products on split operands, and nobody else's.  A bare f32 ops.linear gives the same bits before such an engine's
    forward, after it, and after a bf16 engine's forward that follows; the same product with split=True differs from them."""
    from mgsv_amd import ops
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(300, 256, device="cuda", generator=g)
    w = torch.randn(128, 256, device="cuda", generator=g) / 16
    bias = torch.randn(128, device="cuda", generator=g)
    before = ops.linear(x, w, bias).clone()
    cfg = cfg_native()
    sd = synth.make_state_dict(cfg, seed=0)
    inp = synth.make_inputs(cfg, 2, 20, 40, seed=1)
    MadeEngine(cfg, sd, dtype="f32x3").forward_numpy(inp)
    after = ops.linear(x, w, bias).clone()
    torch.cuda.synchronize()
    assert torch.equal(before, after), float((before - after).abs().max())
    MadeEngine(cfg, sd, dtype="bf16").forward_numpy(inp)
    after_bf16 = ops.linear(x, w, bias).clone()
    split = ops.linear(x, w, bias, split=True).clone()
    torch.cuda.synchronize()
    assert torch.equal(before, after_bf16), float((before - after_bf16).abs().max())
    assert not torch.equal(before, split)                                        # (the two modes do differ on this product: the checks above can fail)


def _device_inputs(cfg, B=2, Tv=20, Ta=40, seed=1):
    inp = synth.make_inputs(cfg, B, Tv, Ta, seed=seed)
    return {k: torch.from_numpy(v).cuda() for k, v in inp.items() if isinstance(v, np.ndarray)}


def test_every_f32_product_of_an_f32x3_engine_is_a_split_one(monkeypatch):
    """Every made_linear / made_attention / made_attention_wide launch of every entry point carries the engine's mode: f32_products = 1 on each
    f32-compute launch of an "f32x3" engine, 0 on each launch of an "f32" engine.  (A call site that bypassed the engine's bound ops would only
    run slower and still meet the 1e-4 gates: this is the test that sees it.)"""
    from mgsv_amd import _lib
    from mgsv_amd.grounding import ground
    l = _lib.lib()
    seen = []                                                                    # (compute dtype, f32_products) of each launch
    for name, dtype_field in (("made_linear", "w_dtype"), ("made_attention", "dtype"), ("made_attention_wide", "dtype")):
        def recording(args, stream, _real=getattr(l, name), _field=dtype_field):
            seen.append((getattr(args._obj, _field), args._obj.f32_products))
            return _real(args, stream)
        monkeypatch.setattr(l, name, recording)
    cfg = cfg_native()
    sd = synth.make_state_dict(cfg, seed=0)
    t = _device_inputs(cfg)
    B = t["frame_feats"].shape[0]
    for dtype, want in (("f32x3", 1), ("f32", 0)):
        eng = MadeEngine(cfg, sd, dtype=dtype)
        V = eng.encode_videos(t["frame_feats"], t["frame_masks"], t["v_duration"])
        M = eng.encode_music(t["segment_feats"], t["segment_masks"])
        entry_points = {
            "forward": lambda: eng.forward(t["frame_feats"], t["segment_feats"], t["frame_masks"], t["segment_masks"], t["spans_target"],
                                           v_duration=t["v_duration"]),
            "retrieval_sim_matrix": lambda: eng.retrieval_sim_matrix(V.vec, M.tokens, M.mask, M.vec),
            "xpool_sims": lambda: eng.xpool_sims(V.vec, M.tokens, M.mask),
            "dual_sims": lambda: eng.dual_sims(V.vec, M.vec),
            "encode_videos": lambda: eng.encode_videos(t["frame_feats"], t["frame_masks"], t["v_duration"]),
            "encode_music": lambda: eng.encode_music(t["segment_feats"], t["segment_masks"]),
            "localize_pairs": lambda: eng.localize_pairs(V, M, torch.arange(B), torch.arange(B)),
            "ground": lambda: ground(eng, V, M, 1),
        }
        for entry, run in entry_points.items():
            del seen[:]
            run()
            torch.cuda.synchronize()
            assert seen, (dtype, entry)                                          # the entry point did go through the recorded launches
            f32 = [mode for compute, mode in seen if compute == _lib.F32]
            assert f32 and all(mode == want for mode in f32), (dtype, entry, seen)
            if dtype == "f32":
                assert all(mode == 0 for _, mode in seen), (entry, seen)


def test_two_engines_of_different_modes_do_not_see_each_other():
    """An "f32" and an "f32x3" engine on the same weights and batch, each on a stream of its own: alternated from one thread, then driven from
    two threads started together, every output of every round is bit for bit what that engine gives alone -- and the two engines' outputs
    differ from each other, so a mode that leaked from one to the other would show.  (The threaded half is the one that discriminates: with a
    mode kept in the library, two threads of different modes race.)"""
    import threading
    cfg = cfg_native()
    sd = synth.make_state_dict(cfg, seed=0)
    t = _device_inputs(cfg)
    keys = ["pred_logits", "pred_spans", "sims_single", "sims_dual", "video_feats", "music_feats"]
    engines = [MadeEngine(cfg, sd, dtype="f32"), MadeEngine(cfg, sd, dtype="f32x3")]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def step(i):
        with torch.cuda.stream(streams[i]):
            o = engines[i].forward(t["frame_feats"], t["segment_feats"], t["frame_masks"], t["segment_masks"], t["spans_target"],
                                   v_duration=t["v_duration"])
            got = {k: o[k].clone() for k in keys}
        streams[i].synchronize()
        return got

    torch.cuda.synchronize()
    solo = [step(0), step(1)]                                                    # (also every launcher's one-time set-up, before any thread)
    assert any(not torch.equal(solo[0][k], solo[1][k]) for k in keys)

    def same(i, got, what):
        for k in keys:
            assert torch.equal(got[k], solo[i][k]), f"{what}, {engines[i].dtype_name}: {k} differs from the engine's solo run"

    for r in range(3):                                                           # one thread, alternating
        for i in range(2):
            same(i, step(i), f"alternating round {r}")

    start = threading.Barrier(2)
    results, errors = [[], []], []

    def drive(i):
        try:
            start.wait()
            for _ in range(3):
                results[i].append(step(i))
        except BaseException as ex:                                              # reported by the test's own thread below
            errors.append((i, ex))

    threads = [threading.Thread(target=drive, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for i in range(2):
        assert len(results[i]) == 3
        for r, got in enumerate(results[i]):
            same(i, got, f"threaded round {r}")
