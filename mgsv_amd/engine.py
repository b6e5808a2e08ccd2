"""Forward executor of the MaDe hot path on MI355X.

`MadeEngine` owns the packed device weights and a shape-keyed workspace and runs the
reference's `Uni_model.forward` (reference model/model_Uni.py:177-322, eval mode) plus the
all-pairs retrieval scoring of reference test-MaDe.py:386-403 as a fixed sequence of kernels
from libmade_hip.so, all on the current HIP stream with no host synchronisation (so the whole
step can be captured in a HIP graph).  PyTorch only provides device memory and the stream.

Data layout in HBM (B = batch, L = T_v + T_a under concat fusion, D = dim_input):
  * activations are row-major [rows, D] in the compute dtype (f32 or bf16), one row per token;
  * the DETR input `fus` [B, L, D] is written in place by the two temporal encoders' last GEMMs
    (frame rows 0..T_v-1, segment rows T_v..L-1) -- the reference's torch.cat never happens;
  * q | k | v of every attention live side by side in one [rows, 3D] buffer written by one GEMM; the
    attention kernels read V row-major and transpose it on the fly (ds_read_b64_tr_b16);
  * the decoder never projects the L memory rows: its cross-attention runs in memory space
    (made_attention_wide over memory + pos) with W_k folded onto the query and W_v / out_proj folded
    into one Linear on the pooled rows (removes 25 % of the forward flops).
"""
from __future__ import annotations

import functools
import math
import os
from dataclasses import dataclass
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import _lib, ops, ops_train
from .config import MadeConfig
from .ops import Seg, round_up

Tensor = torch.Tensor


@dataclass
class Encoded:
    """Per-item tower outputs (MadeEngine.encode_videos / encode_music): tokens [N, T, D] in the compute dtype (any item stride,
    contiguous rows), mask [N, T] f32, vec [N, D] f32 (the L2-normalised clip / track vector), duration [N] f32 seconds or None."""
    tokens: Tensor
    mask: Tensor
    vec: Tensor
    duration: Optional[Tensor] = None

    def __len__(self) -> int:
        return self.tokens.shape[0]


class _Call(NamedTuple):
    """What the stages of one forward, or of one batch of `localize_pairs`, share.  One record per call, never engine state: an engine
    serves two batches in flight."""
    ws: Dict[str, Tensor]                 # MadeEngine._buffers(B, Tv, Ta)
    B: int
    fm: Tensor                            # frame / segment masks [B, Tv] / [B, Ta] f32
    sm: Tensor
    frame: Tensor                         # the towers' token outputs [B, Tv, D] / [B, Ta, D] (views into the workspace)
    seg: Tensor
    video: Tensor                         # clip / track vectors [B, D] f32
    music: Tensor
    pos: Tensor                           # MadeEngine._fused_lists: position embedding and index lists of the fused sequence
    rows_f: tuple
    order_f: Tensor
    v_duration: Optional[Tensor]


class MadeEngine:
    def __init__(self, cfg: MadeConfig, state_dict: Dict[str, object], device="cuda:0", dtype: str = "f32"):
        assert dtype in ("f32", "f32x3", "bf16")
        self.cfg = cfg
        self.device = torch.device(device)
        self.tc = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.dtype_name = dtype
        # "f32x3": f32 storage and elementwise arithmetic like "f32"; the matrix products run as three bf16 products on split operands
        # (f32_products = 1 in each launch's arguments: include/made_hip.h) instead of the exact-f32 MFMA at 1/16 of the bf16 rate.
        # Decided here, once: every matrix product of the engine is issued through these four names.
        self._linear, self._linear_splitk, self._attention, self._attention_wide = ops.linear, ops.linear_splitk, ops.attention, ops.attention_wide
        if dtype == "f32x3":
            self._linear, self._linear_splitk = functools.partial(ops.linear, split=True), functools.partial(ops.linear_splitk, split=True)
            self._attention, self._attention_wide = functools.partial(ops.attention, split=True), functools.partial(ops.attention_wide, split=True)
        self._check_supported()
        self._ws: Dict[tuple, Dict[str, Tensor]] = {}
        self._side: Optional[torch.cuda.Stream] = None       # the second stream, created on first use (_side_stream)
        self.load_state_dict(state_dict)

    # ------------------------------------------------------------------ config support
    def _check_supported(self):
        c = self.cfg
        unsupported = []
        if c.agg_module == "mlp":
            if c.video_transformer_depth != 0 or c.audio_transformer_depth != 0:
                unsupported.append("agg_module=mlp with a temporal transformer depth > 0 (the reference asserts 0, model_Base.py:308)")
        elif "transf" not in c.agg_module or c.video_transformer_depth < 1 or c.audio_transformer_depth < 1:
            unsupported.append(f"agg_module={c.agg_module} / temporal transformer depth 0")
        if "concat" not in c.mml_fusion and "CA" not in c.mml_fusion:
            unsupported.append(f"mml_fusion={c.mml_fusion}")
        if "XA" not in c.vmr_fusion or not ("music" in c.vmr_fusion or "video" in c.vmr_fusion):
            unsupported.append(f"vmr_fusion={c.vmr_fusion}")
        if "music" not in c.vmr_fusion and c.vmr_loss not in ("dual", "single"):
            unsupported.append(f"vmr_loss={c.vmr_loss} without the music-pooling tower (the reference fails there too)")
        if not ("detr" in c.mml_localization or "regression" in c.mml_localization):
            unsupported.append(f"mml_localization={c.mml_localization}")
        if c.audio_short_cut and not c.contrastive_align_loss:
            unsupported.append("audio_short_cut without contrastive_align_loss")
        if c.moment_query_type not in ("video", "music", "zero", "random", "xpool"):
            unsupported.append(f"moment_query_type={c.moment_query_type}")
        if c.moment_query_type == "xpool" and "music" not in c.vmr_fusion:
            unsupported.append("moment_query_type=xpool without the music-pooling tower (the reference fails there too)")
        if c.vmr_loss not in ("dual", "single", "dual_single_loss_fuse", "dual_single_sim_fuse", "dual_single_feature_fuse"):
            unsupported.append(f"vmr_loss={c.vmr_loss}")
        if c.detr_dec_layers < 1:
            unsupported.append("detr_dec_layers=0")
        if c.D not in (128, 256, 512):
            unsupported.append(f"dim_input={c.D} (the wide-head attention kernel is built for 128, 256 and 512)")
        if unsupported:
            raise NotImplementedError("MadeEngine (HIP path) does not cover yet: " + "; ".join(unsupported))

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Dict[str, object]):
        """Pack reference-layout weights for the kernels: matrices in the compute dtype,
        biases / LayerNorm parameters / tables in f32."""
        dev, tc = self.device, self.tc
        c = self.cfg
        D = c.D

        def T(name) -> Tensor:
            v = sd[name]
            t = v.detach().clone() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v).copy())
            return t.to(dev, torch.float32)

        P: Dict[str, Tensor] = {}

        def mat(key, t: Tensor):
            P[key] = t.to(tc).contiguous()

        def vec(key, t: Tensor):
            P[key] = t.to(torch.float32).contiguous()

        def lin(key, name):
            mat(key + ".w", T(name + ".weight"))
            vec(key + ".b", T(name + ".bias"))

        def ln(key, name):
            vec(key + ".g", T(name + ".weight"))
            vec(key + ".b", T(name + ".bias"))

        lin("vit_proj", "vit_proj")
        lin("ast_proj", "ast_proj")
        if c.agg_module == "mlp":                                        # reference model/model_Base.py:216-249,357-377
            for key, mod in (("video_mlp", "Video_encoder_projection"), ("audio_mlp", "Music_encoder_projection")):
                lin(key + ".0", mod + ".net.0"); lin(key + ".3", mod + ".net.3"); lin(key + ".6", mod + ".net.6")
                for bn in ("1", "4"):                                     # eval-mode BatchNorm1d over the token axis -> (scale, shift) per position
                    sc = T(f"{mod}.net.{bn}.weight") / torch.sqrt(T(f"{mod}.net.{bn}.running_var") + 1e-5)
                    vec(f"{key}.{bn}.scale", sc)
                    vec(f"{key}.{bn}.shift", T(f"{mod}.net.{bn}.bias") - T(f"{mod}.net.{bn}.running_mean") * sc)
        else:
            vec("pe_video", T("video_position_embedding.pe")[0])
            vec("pe_audio", T("audio_position_embedding.pe")[0])
            share = bool(c.transformer_is_share) and c.video_transformer_depth == c.audio_transformer_depth
            if c.with_cls_token:                                          # reference model/model_Base.py:314-321
                vec("cls_video", T("video_cls_token").view(-1))
                vec("cls_audio", T("audio_cls_token").view(-1))
            for mod, depth in (("video_transformer", c.video_transformer_depth), ("audio_transformer", c.audio_transformer_depth)):
                src = "share_transformer" if share else mod               # one block for both towers (model_Base.py:322-331)
                for l in range(depth):
                    p, q = f"{mod}.layers.{l}", f"{src}.layers.{l}"
                    ln(p + ".ln1", q + ".0")
                    mat(p + ".in.w", T(q + ".1.in_proj_weight")); vec(p + ".in.b", T(q + ".1.in_proj_bias"))
                    lin(p + ".out", q + ".1.out_proj")
                    ln(p + ".ln2", q + ".2")
                    lin(p + ".ff1", q + ".3.0")
                    lin(p + ".ff2", q + ".3.3")
                lin(mod + ".final", src + ".final_linear")
        towers = []
        if "music" in c.vmr_fusion:
            towers.append(("xa", "video_guided_to_music_pooling_cross_transformer"))
        if "video" in c.vmr_fusion:                                      # reference model/model_Uni.py:26-27
            towers.append(("xav", "music_guided_to_video_pooling_cross_transformer"))
        for key, xa in towers:
            ln(key + ".ln1", xa + ".layer_norm1"); ln(key + ".ln2", xa + ".layer_norm2"); ln(key + ".ln3", xa + ".layer_norm3")
            lin(key + ".q", xa + ".cross_attn.q_proj")
            mat(key + ".kv.w", torch.cat([T(xa + ".cross_attn.k_proj.weight"), T(xa + ".cross_attn.v_proj.weight")], 0))
            vec(key + ".kv.b", torch.cat([T(xa + ".cross_attn.k_proj.bias"), T(xa + ".cross_attn.v_proj.bias")], 0))
            lin(key + ".out", xa + ".cross_attn.out_proj")
            lin(key + ".lin", xa + ".linear_proj")
            # LayerNorm2's affine part and the residual of modules/transformer.py:176 folded into the Linear (float64 on the host), for
            # the retrieval path whose attention kernel emits xhat = (o - mean) * rstd:
            #   x = xhat g2 + b2,  x + (W x + b) = (W + I) diag(g2) xhat + ((W + I) b2 + b)
            W64 = T(xa + ".linear_proj.weight").double().cpu() + torch.eye(D, dtype=torch.float64)
            g2, b2 = T(xa + ".layer_norm2.weight").double().cpu(), T(xa + ".layer_norm2.bias").double().cpu()
            mat(key + ".linf.w", (W64 * g2[None, :]).float().to(dev))
            vec(key + ".linf.b", (W64 @ b2 + T(xa + ".linear_proj.bias").double().cpu()).float().to(dev))
            # W'' 1 of the stored (compute-dtype) W'': made_xpool_sims forms W'' xhat as k1 (W'' o) + k2 (W'' 1) from z = P.(U W''^T)
            vec(key + ".linf.rs", P[key + ".linf.w"].double().sum(1))
        vec("logit_scale", T("logit_scale").view(1))
        if "CA" in c.mml_fusion:                                          # reference model/model_Base.py:99-213
            ca = "video_music_fusion_cross_transformer"
            mat("ca.q.w", T(ca + ".layers.0.0.to_q.weight"))
            mat("ca.kv.w", T(ca + ".layers.0.0.to_kv.weight"))
            lin("ca.out", ca + ".layers.0.0.to_out.0")
            lin("ca.ff1", ca + ".layers.0.1.net.0")
            lin("ca.ff2", ca + ".layers.0.1.net.3")
            ln("ca.lnq", ca + ".attention_query_layer_norms.0")
            ln("ca.lnc", ca + ".attention_context_layer_norms.0")
            ln("ca.lnf", ca + ".ff_layer_norms.0")
            lin("ca.final", ca + ".final_linear")
        for l in range(c.detr_enc_layers):
            p = f"detr_transformer.encoder.layers.{l}"
            mat(p + ".in.w", T(p + ".self_attn.in_proj_weight")); vec(p + ".in.b", T(p + ".self_attn.in_proj_bias"))
            lin(p + ".out", p + ".self_attn.out_proj")
            lin(p + ".ff1", p + ".linear1"); lin(p + ".ff2", p + ".linear2")
            ln(p + ".ln1", p + ".norm1"); ln(p + ".ln2", p + ".norm2")
        if c.detr_pre_norm and c.detr_enc_layers > 0:
            ln("enc.norm", "detr_transformer.encoder.norm")              # (the reference has it with normalize_before only, transformer.py:34)
        H, hd = c.detr_nheads, D // c.detr_nheads
        for l in range(c.detr_dec_layers):
            p = f"detr_transformer.decoder.layers.{l}"
            mat(p + ".sa.in.w", T(p + ".self_attn.in_proj_weight")); vec(p + ".sa.in.b", T(p + ".self_attn.in_proj_bias"))
            lin(p + ".sa.out", p + ".self_attn.out_proj")
            # one query and one key: softmax == 1, so self-attention is out_proj(v_proj(x)); fold both
            # Linears (float64 on the host, once per load)
            sw, sb = T(p + ".self_attn.in_proj_weight").double().cpu(), T(p + ".self_attn.in_proj_bias").double().cpu()
            so, sob = T(p + ".self_attn.out_proj.weight").double().cpu(), T(p + ".self_attn.out_proj.bias").double().cpu()
            mat(p + ".sa.fold.w", (so @ sw[2 * D:]).float().to(dev)); vec(p + ".sa.fold.b", (so @ sb[2 * D:] + sob).float().to(dev))
            # cross-attention in memory space: move W_k onto the query and W_v (with out_proj) onto the pooled rows.
            #   q'_h = W_k,h^T (W_q,h x + b_q,h)            -> one Linear  D -> H*D   (b_k shifts all keys alike: no effect)
            #   out  = sum_h W_o[:, h] W_v,h pooled_h + W_o b_v + b_o -> one Linear H*D -> D
            w, b = T(p + ".multihead_attn.in_proj_weight").double().cpu(), T(p + ".multihead_attn.in_proj_bias").double().cpu()
            wo, bo = T(p + ".multihead_attn.out_proj.weight").double().cpu(), T(p + ".multihead_attn.out_proj.bias").double().cpu()
            wq_h, wk_h, wv_h = w[:D].view(H, hd, D), w[D:2 * D].view(H, hd, D), w[2 * D:].view(H, hd, D)
            mat(p + ".ca.qk.w", torch.einsum("hjn,hjk->hnk", wk_h, wq_h).reshape(H * D, D).float().to(dev))
            vec(p + ".ca.qk.b", torch.einsum("hjn,hj->hn", wk_h, b[:D].view(H, hd)).reshape(H * D).float().to(dev))
            mat(p + ".ca.vo.w", torch.einsum("mhj,hjn->mhn", wo.view(D, H, hd), wv_h).reshape(D, H * D).float().to(dev))
            mat(p + ".ca.v.w", w[2 * D:].float().to(dev)); mat(p + ".ca.o.w", wo.float().to(dev))    # the same two Linears, not folded (fused chain)
            vec(p + ".ca.vo.b", (wo @ b[2 * D:] + bo).float().to(dev))
            lin(p + ".ff1", p + ".linear1"); lin(p + ".ff2", p + ".linear2")
            ln(p + ".ln1", p + ".norm1"); ln(p + ".ln2", p + ".norm2"); ln(p + ".ln3", p + ".norm3")
        ln("dec.norm", "detr_transformer.decoder.norm")
        mat("query_embed", T("decoder_query_embed.weight"))
        if "regression" in c.mml_localization:                           # reference model/model_Uni.py:66-69
            for i in range(3):
                lin(f"reg_mlp.{i}", f"reg_mlp.layers.{i}")
        else:
            lin("class_embed", "class_embed")
            for i in range(3):
                lin(f"span_embed.{i}", f"span_embed.layers.{i}")
                if c.moment_loss:
                    lin(f"moment_embed.{i}", f"moment_embed.layers.{i}")
            if c.contrastive_align_loss:
                lin("proj_q", "contrastive_align_projection_query")
                lin("proj_v", "contrastive_align_projection_vid")
            vec("empty_weight", T("criterion.empty_weight"))
        # constants
        i = torch.arange(D, dtype=torch.float32)
        vec("dim_t", (10000.0 ** (2 * torch.div(i, 2, rounding_mode="floor") / D)).to(dev))
        w_contr = 0.2 if c.contrastive_align_loss else 0.0
        vec("crit_weights", torch.tensor([4.0 if c.l1_loss else 0.0, 1.0, 0.8, 0.0, w_contr], device=dev))
        self.P = P

    def _side_stream(self):
        if _lib.variant_env("MADE_ONE_STREAM", "0") == "1":     # debugging: every branch on the caller's stream, in issue order
            return torch.cuda.current_stream()
        # never the caller's own stream: the framework deals streams out of a pool of 32 in turn, so a stream made earlier (a hipGraph's
        # capture stream, a warm-up's) can be the one this engine was given as its second -- both branches would share it, and the
        # trainer's per-stream weight-gradient workspaces (MadeTrainer._flush_dw) would be looked up under the wrong lane
        cur = torch.cuda.current_stream()
        while self._side is None or self._side == cur:
            self._side = torch.cuda.Stream(device=self.device)
        return self._side

    # ------------------------------------------------------------------ workspace
    def _buffers(self, B: int, Tv: int, Ta: int) -> Dict[str, Tensor]:
        key = (B, Tv, Ta)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        c, dev, tc = self.cfg, self.device, self.tc
        concat = "concat" in c.mml_fusion
        D, L, Q = c.D, (Tv + Ta if concat else Ta), c.num_moment_queries
        F_t, F_d, nd = c.temporal_ffn_dim, c.detr_dim_feedforward, c.detr_dec_layers
        Lmax = max(L, Ta + 1, Tv + 1) if c.with_cls_token else max(L, Ta, Tv)
        Lpad = round_up(Lmax, 64)
        rows = B * Lmax

        def E(*shape, dtype=None):
            return torch.empty(shape, device=dev, dtype=dtype or tc)

        def Z(*shape, dtype=None):
            return torch.zeros(shape, device=dev, dtype=dtype or tc)

        vr = B * (Tv + 1 if c.with_cls_token else Tv)
        ws = dict(
            # private scratch of the video branch (it runs on its own stream beside the audio branch)
            v_x0=E(vr, D), v_x1=E(vr, D), v_x2=E(vr, D), v_x3=E(vr, D), v_xin=E(vr * c.vit_dim), v_qkv=E(vr, 3 * D),
            v_att=E(vr, D), v_ffn=E(vr, F_t),
            fus=E(B, L, D), fus_mask=E(B, L, dtype=torch.float32), pos=E(B, L, D), srcpos=E(B * L, D),
            x0=E(rows, D), x1=E(rows, D), x2=E(rows, D), x3=E(rows, D), xin=E(B * max(Tv * c.vit_dim, Ta * c.ast_dim)),
            qkv=E(rows, 3 * D), att=E(rows, D), ffn=E(rows, max(F_t, F_d)),
            dq_all=E(B * Q, c.detr_nheads * D), dpool=E(B * Q, c.detr_nheads * D),
            dws=E(32 * B * Q * max(D, 256) * 4 * max(1, nd // 4), dtype=torch.float32),   # split-K partials of the skinny GEMMs
            part_o=E(B * 8 * c.detr_nheads * Q * D, dtype=torch.float32), part_ml=E(B * 8 * c.detr_nheads * Q * 4, dtype=torch.float32),
            vmean=E(B, D, dtype=torch.float32), mmean=E(B, D, dtype=torch.float32),
            video=E(B, D, dtype=torch.float32), music=E(B, D, dtype=torch.float32),
            tgt=E(B * Q, D), t1=E(B * Q, D), t2=E(B * Q, D), tx=E(B * Q, D),
            dqkv=E(B * Q, 3 * D), datt=E(B * Q, D),
            dz=E(3, B * Q, D, dtype=torch.float32), dv=E(B * Q, D), dzero=Z(B * Q, D, dtype=torch.float32),   # fused decoder chain: raw (pre-norm) rows
            dffn=E(B * Q, F_d), hs=E(nd, B * Q, D),
            logits=E(nd, B, Q, 2, dtype=torch.float32), spans=E(nd, B, Q, 2, dtype=torch.float32),
            h1=E(nd * B * Q, D), h2=E(nd * B * Q, D),
            sims_single=E(B, B, dtype=torch.float32), sims_dual=E(B, B, dtype=torch.float32), sims_vp_t=E(B, B, dtype=torch.float32),
            ret_loss=E(1, dtype=torch.float32),
            # row gather (valid-token lists) of the video / audio / fused sequences
            rows_v=(E(B * Tv, dtype=torch.int32), E(1, dtype=torch.int32)), rows_a=(E(B * Ta, dtype=torch.int32), E(1, dtype=torch.int32)),
            rows_f=(E(B * L, dtype=torch.int32), E(1, dtype=torch.int32)),
            order_v=E(B, dtype=torch.int32), order_a=E(B, dtype=torch.int32), order_f=E(B, dtype=torch.int32),
        )
        if c.contrastive_align_loss:
            Dc = c.contrastive_hdim
            ws.update(pq_raw=E(nd * B * Q, Dc, dtype=torch.float32), pq=E(nd, B, Q, Dc, dtype=torch.float32),
                      pv_raw=E(B * Tv, Dc, dtype=torch.float32), pv=E(B, Tv, Dc, dtype=torch.float32),
                      vid_sum=E(B, Dc, dtype=torch.float32))
        if not concat:                      # CA fusion: encoders write their own buffers, the fusion block writes `fus`
            inner = c.ca_heads * c.ca_dim_head
            ws.update(frame_buf=E(B, Tv, D), seg_buf=E(B, Ta, D), ca_nx=E(B * Ta, D), ca_nc=E(B * Tv, D),
                      ca_q=E(B * Ta, inner), ca_kv=E(B * Tv, 2 * inner), ca_att=E(B * Ta, inner),
                      ca_x=E(B * Ta, D), ca_h=E(B * Ta, c.ca_ffn_dim), ca_y=E(B * Ta, D))
        self._ws[key] = ws
        return ws

    # ------------------------------------------------------------------ building blocks
    def _mha_block(self, x: Tensor, B: int, T: int, w_in: Tensor, b_in: Tensor, key_mask: Optional[Tensor],
                   ws: Dict[str, Tensor], H: int, pos: Optional[Tensor] = None, skip: Optional[Tensor] = None, rows=None,
                   order: Optional[Tensor] = None) -> Tensor:
        """packed in-proj -> flash attention; x [B*T, D]; q,k from (x + pos), v from x; returns att [B*T, D]."""
        D = self.cfg.D
        qkv = ws["qkv"][:B * T]
        if pos is None:
            self._linear(x, w_in, b_in, out=qkv, rows=rows)
        else:                                       # q and k are projected from x + pos (given precomputed), v from x
            self._linear(x, w_in, b_in, A2=pos, a2_replace=True, rows=rows,
                       segs=[Seg(out=qkv, col_begin=0, use_a2=True), Seg(out=qkv[:, 2 * D:], col_begin=2 * D, ldo=qkv.stride(0))])
        q3 = qkv.view(B, T, 3 * D)
        att = ws["att"][:B * T]
        self._attention(q3[:, :, :D], q3[:, :, D:2 * D], q3[:, :, 2 * D:], att.view(B, T, D), H, key_mask=key_mask,
                      q_skip_mask=key_mask if skip is not None else None, order=order)
        return att

    def _encode(self, feats: Tensor, mask: Tensor, which: str, wsall: Dict[str, Tensor], row_off: int, rows=None, order=None,
                out: Optional[tuple] = None) -> None:
        """reference model/model_Base.py:544-617 -> writes fus[:, row_off:row_off+T] and mean/normalised vector.
        out = (tokens [B, T, D] view with contiguous rows, vector [B, D] f32): write there instead (encode_videos / encode_music)."""
        c, P = self.cfg, self.P
        ws = wsall if which == "audio" else {**wsall, **{k[2:]: v for k, v in wsall.items() if k.startswith("v_")}}
        B, T, Kin = feats.shape
        D = c.D
        proj, mod, pe, depth = (("vit_proj", "video_transformer", "pe_video", c.video_transformer_depth) if which == "video"
                                else ("ast_proj", "audio_transformer", "pe_audio", c.audio_transformer_depth))
        nrow = B * T
        mflat = mask.reshape(-1)
        act = ops.ACT_QUICKGELU if c.with_act_after_proj else ops.ACT_NONE
        if out is not None:
            local = out[0]
        elif "concat" in c.mml_fusion:
            local = ws["fus"][:, row_off:row_off + T]                   # [B, T, D] view
        else:
            local = ws["frame_buf"] if which == "video" else ws["seg_buf"]
        mean, vec = (ws["vmean"], ws["video"]) if which == "video" else (ws["mmean"], ws["music"])
        if out is not None:
            vec = out[1]
        if c.agg_module == "mlp":
            return self._encode_mlp(feats, mask, which, ws, local, mean, vec)
        if c.with_cls_token:
            return self._encode_cls(feats, mask, which, ws, local, vec)
        if P[pe].shape[0] < T:
            raise ValueError(f"{which} position table holds {P[pe].shape[0]} positions < T={T} "
                             "(reference model/model_Base.py:533 raises here too)")
        # padded tokens (mask 0) are never read by a valid token: the GEMMs gather the valid rows only (`rows`), the row kernels
        # and the attention skip them; valid rows are bit-identical to the dense computation
        if self.tc == torch.bfloat16:       # mask + f32->bf16 once, then the direct-to-LDS GEMM
            xin = ops.cast_mask_rows(feats.view(nrow, Kin), mflat, ws["xin"][:nrow * Kin].view(nrow, Kin))
            x = self._linear(xin, P[proj + ".w"], P[proj + ".b"], act=act, R=P[pe][:T], r_row_mod=T, out=ws["x0"][:nrow], rows=rows)
        else:
            x = self._linear(feats.view(nrow, Kin), P[proj + ".w"], P[proj + ".b"], a_row_mask=mflat, act=act,
                           R=P[pe][:T], r_row_mod=T, out=ws["x0"][:nrow], rows=rows)
        x = self._temporal_layers(x, B, T, mask, mod, depth, ws, rows, order)
        self._linear(x, P[mod + ".final.w"], P[mod + ".final.b"], out_row_mask=mflat, tile_skip_mask=mflat,
                   segs=[Seg(out=local, ldo=local.stride(1), rows_per_batch=T, out_batch_stride=local.stride(0))])
        ops.masked_mean(local, mask, out=mean)
        ops.l2norm_rows(mean, out_f32=vec)

    def _temporal_layers(self, x: Tensor, B: int, T: int, mask: Tensor, mod: str, depth: int, ws, rows, order) -> Tensor:
        """reference model/model_Base.py:82-91 without the final Linear; x [B*T, D] in ws["x0"]."""
        c, P = self.cfg, self.P
        nrow = B * T
        mflat = mask.reshape(-1)
        for l in range(depth):
            p = f"{mod}.layers.{l}"
            x1 = ops.layernorm(x, P[p + ".ln1.g"], P[p + ".ln1.b"], out=ws["x1"][:nrow], row_skip=mflat)
            att = self._mha_block(x1, B, T, P[p + ".in.w"], P[p + ".in.b"], mask, ws, c.SA_temporal_heads, skip=mflat, rows=rows, order=order)
            x2 = self._linear(att, P[p + ".out.w"], P[p + ".out.b"], R=x1, out=ws["x2"][:nrow], rows=rows)
            x3 = ops.layernorm(x2, P[p + ".ln2.g"], P[p + ".ln2.b"], out=ws["x3"][:nrow], row_skip=mflat)
            h = self._linear(x3, P[p + ".ff1.w"], P[p + ".ff1.b"], act=ops.ACT_GELU, out=ws["ffn"][:nrow, :c.temporal_ffn_dim], rows=rows)
            x = self._linear(h, P[p + ".ff2.w"], P[p + ".ff2.b"], R=x3, out=ws["x0"][:nrow], rows=rows)
        return x

    def _encode_mlp(self, feats: Tensor, mask: Tensor, which: str, ws, local: Tensor, mean: Tensor, vec: Tensor) -> None:
        """agg_module = "mlp" (reference model/model_Base.py:567-570,606-609 with EmbeddingNet :216-249, eval mode): projection,
        Linear - BatchNorm1d - ReLU - Linear - BatchNorm1d - ReLU - Linear on every token, masked mean.  The BatchNorms' channel
        axis is the token position, so T must equal the length they were built for."""
        c, P = self.cfg, self.P
        B, T, Kin = feats.shape
        key, proj, Tbn = (("video_mlp", "vit_proj", c.max_v_frames) if which == "video" else ("audio_mlp", "ast_proj", c.max_snippet_num))
        if T != Tbn:
            raise ValueError(f"agg_module=mlp: {which} sequence length {T} != {Tbn} positions of its BatchNorm1d (the reference fails there too)")
        nrow = B * T
        mflat = mask.reshape(-1)
        act = ops.ACT_QUICKGELU if c.with_act_after_proj else ops.ACT_NONE
        if self.tc == torch.bfloat16:
            xin = ops.cast_mask_rows(feats.view(nrow, Kin), mflat, ws["xin"][:nrow * Kin].view(nrow, Kin))
            x = self._linear(xin, P[proj + ".w"], P[proj + ".b"], act=act, out=ws["x0"][:nrow])
        else:
            x = self._linear(feats.view(nrow, Kin), P[proj + ".w"], P[proj + ".b"], a_row_mask=mflat, act=act, out=ws["x0"][:nrow])
        h = self._linear(x, P[key + ".0.w"], P[key + ".0.b"], out=ws["ffn"][:nrow, :1024])
        ops.row_affine(h, P[key + ".1.scale"], P[key + ".1.shift"], act=ops.ACT_RELU)
        y = self._linear(h, P[key + ".3.w"], P[key + ".3.b"], out=ws["x1"][:nrow])
        ops.row_affine(y, P[key + ".4.scale"], P[key + ".4.shift"], act=ops.ACT_RELU)
        self._linear(y, P[key + ".6.w"], P[key + ".6.b"], out_row_mask=mflat,
                   segs=[Seg(out=local, ldo=local.stride(1), rows_per_batch=T, out_batch_stride=local.stride(0))])
        ops.masked_mean(local, mask, out=mean)
        ops.l2norm_rows(mean, out_f32=vec)

    def _encode_cls(self, feats: Tensor, mask: Tensor, which: str, ws, local: Tensor, vec: Tensor) -> None:
        """with_cls_token (reference model/model_Base.py:527-530,572-574): a learned token is prepended (its mask entry is 1), the
        block runs on T + 1 positions, the clip vector is the token's output and the local features are the other T rows."""
        c, P = self.cfg, self.P
        B, T, Kin = feats.shape
        D = c.D
        proj, mod, pe, depth, cls = (("vit_proj", "video_transformer", "pe_video", c.video_transformer_depth, "cls_video") if which == "video"
                                     else ("ast_proj", "audio_transformer", "pe_audio", c.audio_transformer_depth, "cls_audio"))
        T1 = T + 1
        if P[pe].shape[0] < T1:
            raise ValueError(f"{which} position table holds {P[pe].shape[0]} positions < T+1={T1} (reference model/model_Base.py:533)")
        mask1 = torch.cat([torch.ones_like(mask[:, :1]), mask], dim=1).contiguous()
        rows1, order1 = self._row_lists(mask1)
        act = ops.ACT_QUICKGELU if c.with_act_after_proj else ops.ACT_NONE
        x = ws["x0"][:B * T1]
        x3d = x.view(B, T1, D)
        x3d[:, 0] = (P[cls] + P[pe][0]).to(self.tc)                      # the token, with position 0's encoding
        seg = Seg(out=x3d[:, 1:], ldo=D, rows_per_batch=T, out_batch_stride=T1 * D)
        if self.tc == torch.bfloat16:
            xin = ops.cast_mask_rows(feats.view(B * T, Kin), mask.reshape(-1), ws["xin"][:B * T * Kin].view(B * T, Kin))
            self._linear(xin, P[proj + ".w"], P[proj + ".b"], act=act, R=P[pe][1:T1], r_row_mod=T, segs=[seg])
        else:
            self._linear(feats.view(B * T, Kin), P[proj + ".w"], P[proj + ".b"], a_row_mask=mask.reshape(-1), act=act,
                       R=P[pe][1:T1], r_row_mod=T, segs=[seg])
        x = self._temporal_layers(x, B, T1, mask1, mod, depth, ws, rows1, order1)
        y = self._linear(x, P[mod + ".final.w"], P[mod + ".final.b"], out_row_mask=mask1.reshape(-1), out=ws["x1"][:B * T1])
        y3 = y.view(B, T1, D)
        ops.l2norm_rows(y3[:, 0], out_f32=vec)
        local.copy_(y3[:, 1:])

    # ------------------------------------------------------------------ X-Pool scoring
    def _xpool_path(self, Nv: int, S: int, D: int, pooled_out: Optional[Tensor]) -> str:
        """Which kernel chain scores Nv videos against tracks of S segments (xpool_sims has the chains)."""
        bf16, knob = self.tc == torch.bfloat16, _lib.variant_env
        if bf16 and D == 256 and pooled_out is None and Nv >= 256:
            return "sims" if S <= 96 and knob("MADE_XPOOL_SIMS", "1") != "0" else "fused"
        if bf16 and D in (256, 512) and S <= 512 and pooled_out is None and Nv >= 256 and knob("MADE_XPOOL_ATTN", "1") != "0":
            return "attention"
        if bf16 and Nv <= 64 and S <= 512 and S * D >= 65536 and D in (256, 512) and knob("MADE_XPOOL_INBATCH", "1") != "0":
            return "inbatch"
        return "wide"

    def _xpool_track_bufs(self, cm: int, S: int, D: int, hoist: bool, fold: bool = False) -> tuple:
        """What `_xpool_tracks` needs for chunks of at most cm tracks: (cm, hoist, fold) and its buffers -- LN1 rows, K, U and (hoist) U after
        the out-projection, [cm*S, D] each, [cm*S, 2D] for the last one under `fold`."""
        E = lambda cols: torch.empty(cm * S, cols, device=self.device, dtype=self.tc)
        return cm, hoist, fold, E(D), E(D), E(D), (E(2 * D if fold else D) if hoist else None)

    def _xpool_tracks(self, tower: str, seg: Tensor, mask: Optional[Tensor], bufs: tuple):
        """The per-track operands of one chunk of tracks, seg [n, S, D] (a view is fine) -> K, U [n, S, D]: LayerNorm 1, then the k | v
        Linear.  hoist: out_proj applied to U here, once per segment (it commutes with the softmax-weighted sum, whose rows sum to 1).
        fold: U is [n, S, 2D], out_proj(u) | W'' out_proj(u) with W'' the folded LayerNorm-2 Linear (load_state_dict, `linf`)."""
        P = self.P
        n, S, D = seg.shape
        _, hoist, fold, s1, kbuf, ubuf, u2 = bufs
        rows = n * S
        skip = mask.reshape(-1) if mask is not None else None           # masked segments are never attended to
        ops.layernorm(seg, P[tower + ".ln1.g"], P[tower + ".ln1.b"], out=s1[:rows], row_skip=skip)   # [n,S,D] view -> compact rows
        self._linear(s1[:rows], P[tower + ".kv.w"], P[tower + ".kv.b"], tile_skip_mask=skip,
                   segs=[Seg(out=kbuf, col_begin=0), Seg(out=ubuf, col_begin=D)])
        if not hoist:
            return kbuf[:rows].view(n, S, D), ubuf[:rows].view(n, S, D)
        self._linear(ubuf[:rows], P[tower + ".out.w"], P[tower + ".out.b"], out=u2[:rows, :D], tile_skip_mask=skip)
        if fold:
            self._linear(u2[:rows, :D], P[tower + ".linf.w"], None, out=u2[:rows, D:], tile_skip_mask=skip)
        return kbuf[:rows].view(n, S, D), u2[:rows].view(n, S, -1)

    def _xpool_chunks(self, tower: str, seg: Tensor, seg_mask: Optional[Tensor], bufs: tuple, pairs) -> None:
        """The walk over the tracks, bufs' cm at a time: their operands, then the path's per-pair stage pairs(m0, n, K, U, mask)."""
        Nm, cm = seg.shape[0], bufs[0]
        for m0 in range(0, Nm, cm):
            n = min(cm, Nm - m0)
            mask = seg_mask[m0:m0 + n] if seg_mask is not None else None
            K, U = self._xpool_tracks(tower, seg[m0:m0 + n], mask, bufs)
            pairs(m0, n, K, U, mask)

    def xpool_sims(self, video: Tensor, seg: Tensor, seg_mask: Tensor, sims_out: Optional[Tensor] = None,
                   pooled_out: Optional[Tensor] = None, chunk_m: Optional[int] = None, tower: str = "xa") -> Tensor:
        """sims[n, m] = <v_n/|v_n|, XA(v, seg, mask)[m, n]/|.|>: reference modules/transformer.py:156-180 +
        modules/metrics.py:10-24.  video [Nv, D] f32; seg [Nm, S, D] (compute dtype, strided ok); mask [Nm, S].
        tower = "xav": the music-guided video pooling block (reference model_Uni.py:203, metrics.py:26-41) -- same
        arithmetic with the roles swapped: pass (music, frames, frame mask) and read the result as sims[m, v].
        Music tracks are processed in chunks so the per-pair intermediates stay bounded."""
        P, tc, dev = self.P, self.tc, self.device
        Nv, D = video.shape
        Nm, S, _ = seg.shape
        if sims_out is None:
            sims_out = torch.empty(Nv, Nm, device=dev, dtype=torch.float32)
        path = self._xpool_path(Nv, S, D, pooled_out)
        v1 = ops.layernorm(video, P[tower + ".ln1.g"], P[tower + ".ln1.b"], out_dtype=tc)
        q = self._linear(v1, P[tower + ".q.w"], P[tower + ".q.b"])
        scale = 1.0 / math.sqrt(D)
        ln2, ln3 = [(P[tower + f".ln{i}.g"], P[tower + f".ln{i}.b"]) for i in (2, 3)]
        E = lambda *shape, dtype=tc: torch.empty(shape, device=dev, dtype=dtype)
        track_bufs = lambda cm, hoist=True, fold=False: self._xpool_track_bufs(cm, S, D, hoist, fold)
        if path in ("sims", "fused"):
            # retrieval scale: the per-pair chain (attention -> LayerNorm2 -> Linear + residual -> LayerNorm3 -> cosine) in one
            # kernel, nothing per pair ever written to HBM (made_xpool_fused); the per-track K / U projections stay GEMMs
            vn = ops.l2norm_rows(video)
            cm = min(Nm, max(1, (2 << 30) // (3 * S * D * tc.itemsize)), 65535)
            bufs = track_bufs(cm, fold=path == "sims")
            if path == "sims":
                # round 4: the per-pair Linear moved onto the values.  W'' o = sum_s p_s (W'' u_s), so u''_s = W'' u_s is made once per
                # segment (one more GEMM over the tracks) and the pair costs a second P.V product (2 S D flops) instead of the Linear (2 D^2):
                # 2.2x fewer flops per pair at S = 96.  The default for tracks of at most 96 segments (made_xpool_sims: 52.5 ms against
                # made_xpool_fused's 60.7-61.3 on the 53 k x 4 k set); MADE_XPOOL_SIMS=0: the fused kernel
                xws = E(ops.xpool_sims_ws_bytes(Nv, cm, D), dtype=torch.uint8)

                def pairs(m0, n, K, UU, mask):
                    ops.xpool_sims(q, K, UU, mask, P[tower + ".linf.b"], P[tower + ".linf.rs"], ln3, vn, sims_out[:, m0:m0 + n], scale=scale,
                                   ws=xws, prepare_ws=(m0 == 0))
            else:
                xws = E(ops.xpool_fused_ws_floats(Nv, cm, D), dtype=torch.float32)

                def pairs(m0, n, K, U, mask):
                    ops.xpool_fused(q, K, U, mask, ln2, P[tower + ".lin.w"], P[tower + ".lin.b"], ln3, vn, sims_out[:, m0:m0 + n], scale=scale,
                                    ws=xws, prepare_ws=(m0 == 0))
        elif path == "attention":
            # retrieval scale at the widths / lengths made_xpool_fused does not serve (D = 512, or more than its segments): the attention
            # as ONE two-pass kernel per chunk of tracks (made_xpool_attention: scores of a whole track in LDS, the normalisation of
            # LayerNorm2 in its tail), then the folded Linear and LayerNorm3 + cosine.  Chunks of about 1 GB of per-pair rows per tensor:
            # measured (tools/retr512_breakdown.py, 8192 x 512 x S 512), chunks small enough to stay in the Infinity Cache lose more to
            # short launches (13.8 ms per pass at 12 tracks per chunk) than they gain (11.45 ms at 96).
            cm = chunk_m if chunk_m is not None else max(1, min(Nm, (1 << 30) // max(Nv * D * tc.itemsize, 1)))
            bufs = track_bufs(cm)
            xh, y, iws = E(cm * Nv, D), E(cm * Nv, D), E(cm * 32, dtype=torch.int32)

            def pairs(m0, n, K, U, mask):
                ops.xpool_attention(q, K, U, mask, xh[:n * Nv].view(n, Nv, D), scale=scale, ws=iws)
                self._linear(xh[:n * Nv], P[tower + ".linf.w"], P[tower + ".linf.b"], out=y[:n * Nv])
                ops.xpool_tail(y[:n * Nv], ln3[0], ln3[1], video, sims_out[:, m0:m0 + n], n, Nv)
        else:
            if chunk_m is None:
                budget = 6 << 30                                         # bytes of per-pair intermediates per chunk
                per_m = Nv * 3 * D * tc.itemsize + 4 * S * D * tc.itemsize
                chunk_m = max(1, min(Nm, budget // max(per_m, 1)))
            cm = min(chunk_m, Nm)
            hoist = Nv > S
            bufs = track_bufs(cm, hoist)
            o, o2, o3 = E(cm * Nv, D), E(cm * Nv, D), E(cm * Nv, D)
            # (no counters in the in-batch workspace since the one-launch form went: nothing to clear)
            xib_ws = E(ops.xpool_inbatch_ws_bytes(cm, S), dtype=torch.uint8) if path == "inbatch" else None

            def pairs(m0, n, K, U, mask):
                # all videos attend to each track's segments: softmax over segments, scores never leave the chip
                rows = n * Nv
                if path == "inbatch":
                    # the in-batch shape (round 4): scores per (track, 128 segments), P.V per (track, 128 columns), bf16 probabilities between them
                    ops.xpool_inbatch(q, K, U, mask, o[:rows].view(n, Nv, D), scale=scale, ws=xib_ws)
                else:
                    # n_split=1: splitting the keys over workgroups + a merge launch is no faster here and costs the other stream CUs
                    # (1.2 % of the eval throughput with two batches in flight)
                    self._attention_wide(q.view(1, Nv, 1, D), K, U, o[:rows].view(n, Nv, 1, D), scale=scale, key_mask=mask, shared_q=True, n_split=1)
                a2 = o[:rows] if hoist else self._linear(o[:rows], P[tower + ".out.w"], P[tower + ".out.b"], out=o2[:rows])
                a3 = ops.layernorm(a2, ln2[0], ln2[1], out=o3[:rows])
                y = self._linear(a3, P[tower + ".lin.w"], P[tower + ".lin.b"], R=a3, out=o2[:rows] if hoist else o[:rows])
                ops.xpool_tail(y, ln3[0], ln3[1], video, sims_out[:, m0:m0 + n], n, Nv,
                               pooled_out=pooled_out[m0 * Nv:(m0 + n) * Nv] if pooled_out is not None else None)
        self._xpool_chunks(tower, seg, seg_mask, bufs, pairs)
        return sims_out

    def xpool_pair_sims(self, video: Tensor, seg: Tensor, seg_mask: Optional[Tensor], start: Tensor, vidx: Tensor, max_count: int = 0,
                        cache: Optional[dict] = None, tower: str = "xa") -> Tensor:
        """The X-Pool similarity of listed pairs, f32 [P]: pair p in [start[u], start[u + 1]) is (video vidx[p], track u of seg) -- `xpool_sims`'
        value for that pair.  video [Nv, D] f32; seg [U, S, D] compute dtype; seg_mask [U, S] or None; start [U + 1] / vidx [P] int32.
        bf16, D = 256, S <= 96: the projections of `xpool_sims`' default path on the U tracks, then one made_xpool_sims_pairs launch (work
        proportional to P).  Everything else: `xpool_sims(video, seg)` -- every video against the U tracks -- and a gather of the listed
        entries: correct everywhere, cheap only when there are few videos.  cache: a dict that keeps the per-video operands between calls
        on the same videos."""
        P, tc, dev = self.P, self.tc, self.device
        Nv, D = video.shape
        U, S, _ = seg.shape
        if not (tc == torch.bfloat16 and D == 256 and S <= 96):
            sims = self.xpool_sims(video, seg, seg_mask, tower=tower)
            col = torch.repeat_interleave(torch.arange(U, device=dev), (start[1:] - start[:-1]).long())
            return sims[vidx.long(), col]
        cache = {} if cache is None else cache
        if "q" not in cache:
            v1 = ops.layernorm(video, P[tower + ".ln1.g"], P[tower + ".ln1.b"], out_dtype=tc)
            cache["q"] = self._linear(v1, P[tower + ".q.w"], P[tower + ".q.b"])
            cache["vn"] = ops.l2norm_rows(video)
        K, UU = self._xpool_tracks(tower, seg, seg_mask, self._xpool_track_bufs(U, S, D, hoist=True, fold=True))
        return ops.xpool_sims_pairs(cache["q"], K, UU, seg_mask, P[tower + ".linf.b"], P[tower + ".linf.rs"],
                                    (P[tower + ".ln3.g"], P[tower + ".ln3.b"]), cache["vn"], start, vidx, scale=1.0 / math.sqrt(D),
                                    max_count=max_count)

    def dual_sims(self, video: Tensor, music: Tensor, out: Optional[Tensor] = None, add: Optional[Tensor] = None, splitk: bool = True) -> Tensor:
        """cos(v, m) (reference modules/loss.py:52-56), always on f32 operands, a bf16 engine's too (exact-f32 MFMA; split products in an "f32x3" engine); `add` is summed in.  splitk False: never the
        in-batch split-K form, whose sums are ordered differently (the shortlist's cosines, which must not depend on the chunking)."""
        vn = ops.l2norm_rows(video)
        mn = ops.l2norm_rows(music)
        Nv, Nm, D = vn.shape[0], mn.shape[0], vn.shape[1]
        if splitk and Nv <= 256 and Nm <= 256 and Nm % 4 == 0 and (add is None or add.stride(0) % 4 == 0):   # in-batch: one output tile -> split K over workgroups
            if out is None:
                out = torch.empty(Nv, Nm, device=vn.device, dtype=torch.float32)
            split = max(2, min(16, D // 32))
            wsp = torch.empty(split * Nv * Nm, device=vn.device, dtype=torch.float32)
            self._linear_splitk(vn, mn, None, wsp, split, R=add, out=out)
            return out
        return self._linear(vn, mn, None, R=add, out=out, out_dtype=torch.float32)

    def retrieval_sim_matrix(self, video_embeds: Tensor, segment_embeds: Tensor, segment_masks: Tensor,
                             music_embeds: Tensor, chunk_m: Optional[int] = None, out: Optional[Tensor] = None,
                             single_out: Optional[Tensor] = None) -> Tensor:
        """reference test-MaDe.py:386-403: sim[Nv, Nm] = single (X-Pool) + dual (cosine).  out / single_out: [Nv, Nm] f32 views
        (two different buffers) that receive the sum / the X-Pool term instead of new tensors."""
        seg = segment_embeds.to(self.tc) if segment_embeds.dtype != self.tc else segment_embeds
        single = self.xpool_sims(video_embeds, seg, segment_masks if self.cfg.fusion_mask == 1 else None, sims_out=single_out, chunk_m=chunk_m)
        return self.dual_sims(video_embeds, music_embeds, out=out, add=single)

    # ------------------------------------------------------------------ full forward
    @torch.no_grad()
    def forward(self, frame_feats: Tensor, segment_feats: Tensor, frame_masks: Tensor, segment_masks: Tensor,
                spans_target: Tensor, with_losses: bool = True, want_pooled: bool = False,
                v_duration: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """reference model/model_Uni.py:177-322 in eval mode.  This function is the schedule only -- which stage runs on which stream and
        who waits for whom (its tail, shared with `localize_pairs`, is `_after_fusion`); the launches are the stages'."""
        c = self.cfg
        if c.predict_center == 1 and v_duration is None:
            raise ValueError("predict_center=1 needs v_duration (reference model/model_Uni.py:280-282)")
        B, Tv, _ = frame_feats.shape
        Ta = segment_feats.shape[1]
        ws = self._buffers(B, Tv, Ta)
        fm, sm = frame_masks.contiguous(), segment_masks.contiguous()
        concat = "concat" in c.mml_fusion
        # the temporal encoders (K1-K4) write straight into the fused DETR input
        frame, seg = (ws["fus"][:, :Tv], ws["fus"][:, Tv:]) if concat else (ws["frame_buf"], ws["seg_buf"])

        # The video branch (B*T_v rows: every launch far smaller than the chip) runs on a second HIP stream beside the audio branch and
        # joins before X-Pool.  The audio branch (the launches that fill the chip) is enqueued first, the video branch (17 launches of
        # at most a few hundred workgroups) second: eager launching is 1-3 % faster this way, graph replay unchanged.
        cur, side = torch.cuda.current_stream(), self._side_stream()
        side.wait_stream(cur)
        self._encode(segment_feats.contiguous(), sm, "audio", ws, Tv, *self._row_lists(sm, ws, "a"))
        with torch.cuda.stream(side):
            lists = self._fused_lists(ws, fm, sm)                # (they depend on the masks only: off the critical path)
            self._encode(frame_feats.contiguous(), fm, "video", ws, 0, *self._row_lists(fm, ws, "v"))
        cur.wait_stream(side)
        k = _Call(ws, B, fm, sm, frame, seg, ws["video"], ws["music"], *lists, v_duration)
        if not concat:
            self._ca_fusion(ws, frame, seg, fm, sm, B, Tv, Ta)
        out: Dict[str, Tensor] = dict(video_feats=k.video, music_feats=k.music, frame_feats=frame, segment_feats=seg)

        # X-Pool similarities + retrieval loss (K5-K7): independent of the DETR branch, so they run on the side stream beside the
        # (latency-bound) decoder and join at the end of the step
        side.wait_stream(cur)
        dec_early = None
        with torch.cuda.stream(side):
            if "regression" not in c.mml_localization and c.moment_query_type != "xpool" and not c.detr_pre_norm:
                # The query side of decoder layer 0 (initial queries -> self-attention block -> the folded cross-attention
                # query) reads nothing the DETR encoder produces: it runs here, beside the encoder, instead of at the head of
                # the decoder's chain of dependent launches.
                self._dec_open(k, None)
                dec_early = torch.cuda.Event()
                dec_early.record(side)
            need_pooled = want_pooled or c.moment_query_type == "xpool" or c.vmr_loss == "dual_single_feature_fuse"
            pooled = torch.empty(B * B, c.D, device=self.device, dtype=torch.float32) if (need_pooled and "music" in c.vmr_fusion) else None
            out.update(self._retrieval(k, pooled, with_losses))
        if pooled is not None:
            out["music_feats_pooled"] = pooled.view(B, B, c.D)
        return self._after_fusion(k, out, cur, side, dec_early=dec_early, pooled=pooled, spans_target=spans_target, with_losses=with_losses)

    def _after_fusion(self, k: "_Call", out: Dict[str, Tensor], cur, side, *, dec_early=None, pooled: Optional[Tensor] = None,
                      spans_target: Optional[Tensor] = None, with_losses: bool = False) -> Dict[str, Tensor]:
        """The schedule after the towers and the fusion (K8-K14), on the fused input ws["fus"] / ws["fus_mask"]: `forward`'s tail, and a
        batch of `localize_pairs` (no second stream there: side is cur).  dec_early: the event of decoder layer 0's query side when it
        already ran beside the encoder (forward's side stream), else None."""
        c = self.cfg
        regression = "regression" in c.mml_localization
        out["memory"] = memory = self._detr_encoder(k, all_rows=regression)
        if regression:
            out.update(self._regression_head(k, memory, spans_target, with_losses))
        else:
            if dec_early is not None:
                cur.wait_event(dec_early)                    # layer 0's query side was computed beside the encoder
            else:
                if c.moment_query_type == "xpool":           # reference model_Uni.py:222-223: the track's pooled vectors, averaged
                    cur.wait_stream(side)                    # over the videos of the batch (X-Pool branch first)
                self._dec_open(k, pooled)
            out.update(self._decoder(k, memory))
            out.update(self._heads(k))
            if with_losses:
                out.update(self._criterion(k, spans_target))
        cur.wait_stream(side)
        return out

    # ------------------------------------------------------------------ stages (they touch no stream)
    def _row_lists(self, mask: Tensor, ws=None, tag: str = "") -> tuple:
        """(rows, order) of a token mask [B, T]: the valid-row list the GEMMs gather by, and the samples by descending length (attention
        workgroups: longest sample first).  Into ws["rows_" + tag] / ws["order_" + tag] when a workspace is given."""
        out_r, out_o = (ws["rows_" + tag], ws["order_" + tag]) if ws is not None else (None, None)
        return ops.row_index(mask, out=out_r), ops.batch_order(mask, out=out_o)

    def _fused_lists(self, ws, fm: Tensor, sm: Tensor) -> tuple:
        """The DETR token mask ws["fus_mask"], then (pos, rows_f, order_f): its sine position embedding and its index lists."""
        fus_mask = ops.concat_cols(fm if "concat" in self.cfg.mml_fusion else None, sm, ws["fus_mask"])
        pos = ops.sine_pe(fus_mask, self.P["dim_t"], out=ws["pos"])
        return (pos, *self._row_lists(fus_mask, ws, "f"))

    def _retrieval(self, k: "_Call", pooled: Optional[Tensor], with_losses: bool) -> Dict[str, Tensor]:
        """Retrieval branch: the X-Pool tower(s), the dual cosine similarities, (with_losses) the retrieval loss.  Returns its outputs."""
        c, ws = self.cfg, k.ws
        out: Dict[str, Tensor] = {}
        if "music" in c.vmr_fusion:
            self.xpool_sims(k.video, k.seg, k.sm if c.fusion_mask == 1 else None, sims_out=ws["sims_single"], pooled_out=pooled)
        if "video" in c.vmr_fusion:
            # music-guided video pooling (reference model_Uni.py:203, metrics.py:26-41): the same block with the roles
            # swapped gives sims[m, v]; the reference adds its transpose to the music-pooling similarities (:247-251)
            vp = self.xpool_sims(k.music, k.frame, k.fm if c.fusion_mask == 1 else None, sims_out=ws["sims_vp_t"], tower="xav")
            out["sims_video_pooling"] = vp.t()
            if "music" in c.vmr_fusion:
                ws["sims_single"].add_(vp.t())
            else:
                ws["sims_single"].copy_(vp.t())
        self.dual_sims(k.video, k.music, out=ws["sims_dual"])
        out.update(sims_single=ws["sims_single"], sims_dual=ws["sims_dual"])
        if with_losses:
            self._retrieval_loss(ws, k.video, k.music, pooled=pooled)
            out["retrieval_loss"] = ws["ret_loss"]
        return out

    def _detr_encoder(self, k: "_Call", all_rows: bool) -> Tensor:
        """DETR encoder (K8, K9) over ws["fus"] + position embedding -> the memory [B, L, D]; ws["srcpos"] holds memory + pos, the
        decoder's keys.  all_rows: padded positions are computed too -- the regression head sums the memory over ALL of them (reference
        model_Uni.py:229); otherwise padded tokens of the fused sequence are skipped everywhere."""
        c, P, ws = self.cfg, self.P, k.ws
        B, L, D = ws["fus"].shape
        rows, n_layers = B * L, c.detr_enc_layers
        x, pos2, srcpos = ws["fus"].view(rows, D), k.pos.view(rows, D), ws["srcpos"]
        fskip, enc_rows = (None, None) if all_rows else (ws["fus_mask"].view(-1), k.rows_f)
        final_norm = c.detr_pre_norm and n_layers > 0     # (the reference has it with normalize_before only, transformer.py:33-35,107-108)
        if not final_norm:
            ops.layernorm_add(x, None, None, pos2, None, srcpos, row_skip=fskip)      # src + pos (no norm): layer 0's q / k input
        layer = self._enc_layer_pre_norm if c.detr_pre_norm else self._enc_layer_post_norm
        for l in range(n_layers):
            x = layer(k, l, x, fskip, enc_rows)
        if final_norm:
            x, last = ws["x3"][:rows], x
            ops.layernorm_add(last, P["enc.norm.g"], P["enc.norm.b"], pos2, x, srcpos, row_skip=fskip)
        return x.view(B, L, D)

    def _enc_layer_post_norm(self, k: "_Call", l: int, src: Tensor, fskip, enc_rows) -> Tensor:
        """reference music_detr/transformer.py:153-168 (forward_post); reads ws["srcpos"] = src + pos and leaves the next one there."""
        c, P, ws = self.cfg, self.P, k.ws
        B, L, D = ws["fus"].shape
        rows = B * L
        p = f"detr_transformer.encoder.layers.{l}"
        att = self._mha_block(src, B, L, P[p + ".in.w"], P[p + ".in.b"], ws["fus_mask"], ws, c.detr_nheads, pos=ws["srcpos"], skip=fskip,
                              rows=enc_rows, order=k.order_f)
        x = self._linear(att, P[p + ".out.w"], P[p + ".out.b"], R=src, out=ws["x1"][:rows], rows=enc_rows)
        s1 = ops.layernorm(x, P[p + ".ln1.g"], P[p + ".ln1.b"], out=ws["x2"][:rows], row_skip=fskip)
        h = self._linear(s1, P[p + ".ff1.w"], P[p + ".ff1.b"], act=ops.ACT_RELU, out=ws["ffn"][:rows, :c.detr_dim_feedforward], rows=enc_rows)
        x = self._linear(h, P[p + ".ff2.w"], P[p + ".ff2.b"], R=s1, out=ws["x1"][:rows], rows=enc_rows)
        # the norm that produces the next src also emits src + pos (next layer's q/k input, decoder's keys)
        src = ws["x3" if l % 2 == 0 else "x0"][:rows]
        ops.layernorm_add(x, P[p + ".ln2.g"], P[p + ".ln2.b"], k.pos.view(rows, D), src, ws["srcpos"], row_skip=fskip)
        return src

    def _enc_layer_pre_norm(self, k: "_Call", l: int, x: Tensor, fskip, enc_rows) -> Tensor:
        """reference music_detr/transformer.py:170-189 (forward_pre): the residual stream x is never normalised inside a layer; norm 1 feeds
        the attention (q = k = LN1(x) + pos, v = LN1(x)), norm 2 the FFN."""
        c, P, ws = self.cfg, self.P, k.ws
        B, L, D = ws["fus"].shape
        rows = B * L
        p = f"detr_transformer.encoder.layers.{l}"
        n1, srcpos = ws["x2"][:rows], ws["srcpos"]
        ops.layernorm_add(x, P[p + ".ln1.g"], P[p + ".ln1.b"], k.pos.view(rows, D), n1, srcpos, row_skip=fskip)
        att = self._mha_block(n1, B, L, P[p + ".in.w"], P[p + ".in.b"], ws["fus_mask"], ws, c.detr_nheads, pos=srcpos, skip=fskip,
                              rows=enc_rows, order=k.order_f)
        xa = self._linear(att, P[p + ".out.w"], P[p + ".out.b"], R=x, out=ws["x1"][:rows], rows=enc_rows)
        n2 = ops.layernorm(xa, P[p + ".ln2.g"], P[p + ".ln2.b"], out=ws["x2"][:rows], row_skip=fskip)
        h = self._linear(n2, P[p + ".ff1.w"], P[p + ".ff1.b"], act=ops.ACT_RELU, out=ws["ffn"][:rows, :c.detr_dim_feedforward], rows=enc_rows)
        return self._linear(h, P[p + ".ff2.w"], P[p + ".ff2.b"], R=xa, out=ws["x0"][:rows], rows=enc_rows)

    def _dec_open(self, k: "_Call", pooled: Optional[Tensor]) -> None:
        """The initial decoder queries and layer 0 up to its cross-attention: what the decoder reads of the towers only.  (The pre-norm
        layer has its self-attention block inside: there the queries alone.)"""
        ws = k.ws
        if self._fused_decoder():
            self._dec_fused_query_side(ws, 0, self._dec_first_rows(ws, k.video, k.music))
            return
        self._decoder_queries(ws, k.video, k.music, pooled, k.B)
        if not self.cfg.detr_pre_norm:
            self._decoder_query_side(ws, 0, k.B)

    def _decoder(self, k: "_Call", memory: Tensor) -> Dict[str, Tensor]:
        """DETR decoder (K10) behind `_dec_open` -> hs.  Cross-attention runs in memory space (made_attention_wide): no projection of
        the L memory rows at all; self-attention collapses to one folded Linear when there is a single query."""
        c = self.cfg
        layer = self._dec_layer_pre_norm if c.detr_pre_norm else (self._dec_layer_fused if self._fused_decoder() else self._dec_layer_splitk)
        for l in range(c.detr_dec_layers):
            layer(k, l, memory)
        return dict(hs=k.ws["hs"].view(c.detr_dec_layers, k.B, c.num_moment_queries, c.D))

    def _dec_self_attn(self, ws, l: int, x: Tensor, B: int, **to) -> None:
        """Self-attention block of decoder layer l over the queries x [B*Q, D]: one folded Linear when Q = 1, else qkv (q, k from
        x + query_pos) -> attention -> out_proj.  to: the last Linear's residual and outputs (R=, out= or ln1=, ln1_out=)."""
        c, P = self.cfg, self.P
        Q, D = c.num_moment_queries, c.D
        p = f"detr_transformer.decoder.layers.{l}"
        if Q == 1:
            return self._skinny(ws, x, p + ".sa.fold", **to)
        dqkv = ws["dqkv"]
        self._linear(x, P[p + ".sa.in.w"], P[p + ".sa.in.b"], A2=P["query_embed"], a2_row_mod=Q,
                   segs=[Seg(out=dqkv, col_begin=0, use_a2=True), Seg(out=dqkv[:, 2 * D:], col_begin=2 * D, ldo=dqkv.stride(0))])
        d3 = dqkv.view(B, Q, 3 * D)
        self._attention(d3[:, :, :D], d3[:, :, D:2 * D], d3[:, :, 2 * D:], ws["datt"].view(B, Q, D), c.detr_nheads)
        self._skinny(ws, ws["datt"], p + ".sa.out", **to)

    def _dec_cross_attn(self, k: "_Call", memory: Tensor) -> None:
        """ws["dq_all"] (the queries folded with W_k per head) against memory + pos, values = memory -> ws["dpool"], both [B*Q, H*D]."""
        c, ws = self.cfg, k.ws
        B, Q, H, D = k.B, c.num_moment_queries, c.detr_nheads, c.D
        heads = lambda t: t.view(B, Q, H, D).permute(0, 2, 1, 3)         # [B, H, Q, D] view: row (b,q), head-major columns
        self._attention_wide(heads(ws["dq_all"]), ws["srcpos"].view(memory.shape), memory, heads(ws["dpool"]), scale=1.0 / math.sqrt(D // H),
                           key_mask=ws["fus_mask"], n_split=max(1, min(8, 256 // max(B, 1))), part_o=ws["part_o"], part_ml=ws["part_ml"])

    def _dec_layer_pre_norm(self, k: "_Call", l: int, memory: Tensor) -> None:
        """reference music_detr/transformer.py:246-271 (forward_pre): tgt is the un-normalised residual stream; every branch reads a
        norm of it.  The self-attention always runs here.  hs[l] = decoder.norm(tgt after the layer) (:135-136)."""
        P, ws = self.P, k.ws
        p = f"detr_transformer.decoder.layers.{l}"
        skinny = lambda A, wkey, **kw: self._skinny(ws, A, wkey, **kw)
        t1, t2 = ws["t1"], ws["t2"]
        ta, tb = ws["dz"][0], ws["dz"][1]                     # (f32 rows: the stream is rounded to the compute dtype nowhere)
        tcur = ws["tgt"] if l == 0 else ws["dz"][2]
        ops.layernorm(tcur, P[p + ".ln1.g"], P[p + ".ln1.b"], out=t1)
        self._dec_self_attn(ws, l, t1, k.B, R=tcur, out=ta)
        ops.layernorm(ta, P[p + ".ln2.g"], P[p + ".ln2.b"], out=t2)
        skinny(t2, p + ".ca.qk", A2=P["query_embed"], a2_row_mod=self.cfg.num_moment_queries, out=ws["dq_all"])
        self._dec_cross_attn(k, memory)
        skinny(ws["dpool"], p + ".ca.vo", R=ta, out=tb)
        ops.layernorm(tb, P[p + ".ln3.g"], P[p + ".ln3.b"], out=t1)
        skinny(t1, p + ".ff1", act=ops.ACT_RELU, out=ws["dffn"])
        skinny(ws["dffn"], p + ".ff2", R=tb, out=ws["dz"][2], ln1=(P["dec.norm.g"], P["dec.norm.b"]), ln1_out=ws["hs"][l])

    def _dec_layer_fused(self, k: "_Call", l: int, memory: Tensor) -> None:
        """Fused chain (made_dec_stage): every LayerNorm runs in the prologue of the Linear that consumes it, so a layer is
        8 launches instead of 12 and no split-K partial sums go through HBM.  z[0..2]: the raw rows before norm 1 / 2 / 3."""
        c, P, ws = self.cfg, self.P, k.ws
        p = f"detr_transformer.decoder.layers.{l}"
        D, H, nd, rows = c.D, c.detr_nheads, c.detr_dec_layers, k.B * c.num_moment_queries
        z, hd, dv, dpool, t2 = ws["dz"], D // H, ws["dv"], ws["dpool"], ws["t2"]
        if l > 0:
            self._dec_fused_query_side(ws, l, None)
        self._dec_cross_attn(k, memory)
        self._linear(dpool[:, :D], P[p + ".ca.v.w"][:hd], None, M=rows, N=hd, K=D, batch=H, a_z_stride=D, w_z_stride=hd * D,
                   segs=[Seg(out=dv, ldo=D, out_z_stride=hd)])                       # v_h = W_v,h pooled_h (b_v rides in ca.vo.b)
        self._linear(dv, P[p + ".ca.o.w"], P[p + ".ca.vo.b"], R=ws["t1"], out=z[1])
        ops.dec_stage(z[1], P[p + ".ff1.w"], P[p + ".ff1.b"], ws["dffn"], ln=(P[p + ".ln2.g"], P[p + ".ln2.b"]), x_out=t2, act=ops.ACT_RELU)
        self._linear(ws["dffn"], P[p + ".ff2.w"], P[p + ".ff2.b"], R=t2, out=z[2])
        if l == nd - 1:                                      # the last layer's norms have no consumer stage: one row kernel
            ops.splitk_finish(z[2].view(-1), 1, rows, D, None, ln1=(P[p + ".ln3.g"], P[p + ".ln3.b"]), ln1_out=ws["tgt"],
                              ln2=(P["dec.norm.g"], P["dec.norm.b"]), ln2_out=ws["hs"][l])

    def _dec_layer_splitk(self, k: "_Call", l: int, memory: Tensor) -> None:
        """Post-norm layer as split-K Linears with the LayerNorms in their finishing pass (f32 parity mode, Q > 1, the pooled-track query)."""
        P, ws = self.P, k.ws
        p = f"detr_transformer.decoder.layers.{l}"
        ln2, ln3 = [(P[p + f".ln{i}.g"], P[p + f".ln{i}.b"]) for i in (2, 3)]
        t1, t2 = ws["t1"], ws["t2"]
        if l > 0:
            self._decoder_query_side(ws, l, k.B)
        self._dec_cross_attn(k, memory)
        self._skinny(ws, ws["dpool"], p + ".ca.vo", R=t1, ln1=ln2, ln1_out=t2)
        self._skinny(ws, t2, p + ".ff1", act=ops.ACT_RELU, out=ws["dffn"])
        self._skinny(ws, ws["dffn"], p + ".ff2", R=t2, ln1=ln3, ln1_out=ws["tgt"], ln2=(P["dec.norm.g"], P["dec.norm.b"]), ln2_out=ws["hs"][l])

    def _short_cut(self, raw: Tensor, normed: Tensor, mq: Tensor, out: Optional[Tensor] = None) -> Tensor:
        """audio_short_cut (reference model/model_Uni.py:144-145): normalize(normed + music), the sum through `raw`.  mq: `_music_per_query`."""
        ops_train.add3(raw, normed, mq, b_mod=mq.numel())
        return ops.l2norm_rows(raw, out_f32=out)

    def _music_per_query(self, k: "_Call") -> Tensor:
        Q = self.cfg.num_moment_queries
        return k.music if Q == 1 else k.music[:, None, :].expand(k.B, Q, self.cfg.D).contiguous()

    def _heads(self, k: "_Call") -> Dict[str, Tensor]:
        """Heads (K11) on all decoder layers at once: class, span, the contrastive projections, the moment head.  (Running the class head
        and the query projection on the side stream beside the span head was tried: +150 us per step under graph replay, so the three
        chains stay on one stream.)"""
        c, P, ws = self.cfg, self.P, k.ws
        B, Tv, nd = k.B, k.frame.shape[1], c.detr_dec_layers
        hs = ws["hs"]
        hs2 = hs.view(-1, c.D)                                           # [nd * B * Q, D]
        logits, spans = ws["logits"], ws["spans"]
        self._linear(hs2, P["class_embed.w"], P["class_embed.b"], out=logits.view(-1, 2))
        if c.contrastive_align_loss:
            pq_raw, pq2 = ws["pq_raw"], ws["pq"].view(hs2.shape[0], -1)
            self._linear(hs2, P["proj_q.w"], P["proj_q.b"], out=pq_raw)
            ops.l2norm_rows(pq_raw, out_f32=pq2)
            if c.audio_short_cut:
                mq = self._music_per_query(k)
                self._short_cut(pq_raw, pq2, mq, out=pq2)
                if c.aux_loss and nd > 1:
                    # the auxiliary layers get the short-cut a SECOND time when their output dicts are built (reference
                    # model/model_Uni.py:166-169 adds the music vector to the already short-cut proj_queries[:-1])
                    n_aux = (nd - 1) * B * c.num_moment_queries
                    self._short_cut(pq_raw[:n_aux], pq2[:n_aux], mq, out=pq2[:n_aux])
        if hs2.shape[0] <= 1024:
            self._skinny(ws, hs2, "span_embed.0", act=ops.ACT_RELU, out=ws["h1"])
            self._skinny(ws, ws["h1"], "span_embed.1", act=ops.ACT_RELU, out=ws["h2"])
            h2 = ws["h2"]
        else:
            h1 = self._linear(hs2, P["span_embed.0.w"], P["span_embed.0.b"], act=ops.ACT_RELU, out=ws["h1"])
            h2 = self._linear(h1, P["span_embed.1.w"], P["span_embed.1.b"], act=ops.ACT_RELU, out=ws["h2"])
        if c.predict_center == 1:
            # the head predicts the centre only; the width is the video's share of the longest track (reference
            # model/model_Uni.py:135-136,280-282)
            self._linear(h2, P["span_embed.2.w"], P["span_embed.2.b"], act=ops.ACT_SIGMOID, segs=[Seg(out=spans.view(-1, 2), ldo=2)])
            spans[..., 1] = (k.v_duration.to(self.device, torch.float32) / c.max_m_duration).view(1, B, 1)
        else:
            self._linear(h2, P["span_embed.2.w"], P["span_embed.2.b"], act=ops.ACT_SIGMOID, out=spans.view(-1, 2))
        out = dict(pred_logits=logits[-1], pred_spans=spans[-1], logits_all=logits, spans_all=spans)
        if c.contrastive_align_loss:
            self._frame_rows_linear(k.frame, P["proj_v.w"], P["proj_v.b"], ws["pv_raw"], B, Tv)
            pv = ws["pv"]
            ops.l2norm_rows(ws["pv_raw"], out_f32=pv.view(B * Tv, -1))
            ops.masked_mean(pv, None, out=ws["vid_sum"])
            out.update(proj_queries=ws["pq"][-1], proj_vid_mem=pv, proj_queries_all=ws["pq"])
        if c.moment_loss:                                                # reference model_Uni.py:152-159 (outputs only: no loss reads them)
            m1 = self._linear(hs[nd - 1], P["moment_embed.0.w"], P["moment_embed.0.b"], act=ops.ACT_RELU)
            m2 = self._linear(m1, P["moment_embed.1.w"], P["moment_embed.1.b"], act=ops.ACT_RELU)
            m3 = self._linear(m2, P["moment_embed.2.w"], P["moment_embed.2.b"], out_dtype=torch.float32)
            mf = ops.l2norm_rows(m3)
            if c.audio_short_cut:
                mf = self._short_cut(m3, mf, self._music_per_query(k))
            out["moment_feats"] = mf.view(B, c.num_moment_queries, c.D)
        return out

    def _criterion(self, k: "_Call", spans_target: Tensor) -> Dict[str, Tensor]:
        """Matcher + set criterion (K12-K14) on the heads' outputs in the workspace, all layers in one launch each."""
        c, P, ws = self.cfg, self.P, k.ws
        nd, B, Q = c.detr_dec_layers, k.B, c.num_moment_queries
        logits, spans = ws["logits"], ws["spans"]
        pq, vid_sum = (ws["pq"], ws["vid_sum"]) if c.contrastive_align_loss else (None, None)
        tg = spans_target.contiguous()
        pi, ti, cnt, status, cost = ops.hungarian_match(logits.view(nd * B, Q, 2), spans.view(nd * B, Q, 2), tg, c.foreground_label)
        losses, total = ops.set_criterion(logits, spans, tg, pi, ti, cnt, pq, vid_sum, P["empty_weight"],
                                          c.foreground_label, P["crit_weights"])
        return dict(matcher_pred_idx=pi.view(nd, B, -1), matcher_tgt_idx=ti.view(nd, B, -1), matcher_count=cnt.view(nd, B),
                    matcher_status=status, criterion_losses=losses, localization_loss=total)

    # ------------------------------------------------------------------ grounding: towers once per item, localization per pair
    @torch.no_grad()
    def encode_videos(self, frame_feats: Tensor, frame_masks: Tensor, v_duration: Optional[Tensor] = None, batch: int = 64) -> "Encoded":
        """The video temporal tower only (no X-Pool, no DETR) over [N, T_v, vit_dim] features, `batch` items per launch sequence."""
        return self._encode_items(frame_feats, frame_masks, v_duration, "video", batch)

    @torch.no_grad()
    def encode_music(self, segment_feats: Tensor, segment_masks: Tensor, m_duration: Optional[Tensor] = None, batch: int = 64) -> "Encoded":
        """The music temporal tower only over [N, T_a, ast_dim] features."""
        return self._encode_items(segment_feats, segment_masks, m_duration, "audio", batch)

    def _encode_items(self, feats: Tensor, masks: Tensor, duration: Optional[Tensor], which: str, batch: int) -> "Encoded":
        dev, D = self.device, self.cfg.D
        N, T, _ = feats.shape
        feats = feats.to(dev, torch.float32).contiguous()
        masks = masks.to(dev, torch.float32).contiguous()
        rec = Encoded(tokens=torch.empty(N, T, D, device=dev, dtype=self.tc), mask=masks,
                      vec=torch.empty(N, D, device=dev, dtype=torch.float32),
                      duration=duration.to(dev, torch.float32).contiguous() if duration is not None else None)
        for n0 in range(0, N, batch):
            B = min(batch, N - n0)
            m = masks[n0:n0 + B]
            ws = self._buffers(B, T, 1) if which == "video" else self._buffers(B, 1, T)
            rows, order = self._row_lists(m, ws, which[0])
            self._encode(feats[n0:n0 + B], m, which, ws, 0, rows=rows, order=order, out=(rec.tokens[n0:n0 + B], rec.vec[n0:n0 + B]))
        return rec

    def _localize_chunks(self, videos: "Encoded", music: "Encoded", vi: Tensor, mi: Tensor, pair_batch: int):
        """Yields (p0, n, out) per batch of pairs: out["pred_logits"] / out["pred_spans"] of pairs p0 .. p0+n-1 are views into the
        engine's workspace, valid until the next batch is launched.  A short last batch is padded with copies of its last pair
        (pairs are independent: the padding changes no other pair's result) so that every batch uses the same workspace."""
        c = self.cfg
        if c.moment_query_type == "xpool":
            raise NotImplementedError("moment_query_type=xpool: the decoder query is the track's pooled vector averaged over the videos of "
                                      "the batch (reference model/model_Uni.py:222-223), a property of the batch with no per-pair meaning")
        if c.predict_center == 1 and videos.duration is None:
            raise ValueError("predict_center=1 needs the videos' durations (encode_videos(..., v_duration=...))")
        dev = self.device
        vi = torch.as_tensor(vi).to(dev, torch.int32).reshape(-1).contiguous()
        mi = torch.as_tensor(mi).to(dev, torch.int32).reshape(-1).contiguous()
        P = vi.numel()
        assert mi.numel() == P and videos.tokens.dtype == music.tokens.dtype == self.tc
        if P == 0:
            return
        B = max(1, min(pair_batch, P))
        if P % B:
            pad = B - P % B
            vi = torch.cat([vi, vi[-1:].expand(pad)]).contiguous()
            mi = torch.cat([mi, mi[-1:].expand(pad)]).contiguous()
        Tv, Ta = videos.tokens.shape[1], music.tokens.shape[1]
        concat = "concat" in c.mml_fusion
        ws = self._buffers(B, Tv, Ta)
        if "pair_fm" not in ws:
            ws["pair_fm"] = torch.empty(B, Tv, device=dev, dtype=torch.float32)
            ws["pair_sm"] = torch.empty(B, Ta, device=dev, dtype=torch.float32)
        fm, sm, fus = ws["pair_fm"], ws["pair_sm"], ws["fus"]
        video, music_v = ws["video"], ws["music"]
        frame, seg = (fus[:, :Tv], fus[:, Tv:]) if concat else (ws["frame_buf"], ws["seg_buf"])
        cur = torch.cuda.current_stream()
        for p0 in range(0, P, B):
            ops.gather_pairs(vi[p0:p0 + B], mi[p0:p0 + B], videos.tokens, videos.mask, videos.vec, music.tokens, music.mask, music.vec,
                             frame, seg, fm, sm, video, music_v)
            lists = self._fused_lists(ws, fm, sm)
            if not concat:
                self._ca_fusion(ws, frame, seg, fm, sm, B, Tv, Ta)
            vdur = videos.duration[vi[p0:p0 + B].long()] if c.predict_center == 1 else None
            k = _Call(ws, B, fm, sm, frame, seg, video, music_v, *lists, vdur)
            out: Dict[str, Tensor] = dict(video_feats=video, music_feats=music_v, frame_feats=frame, segment_feats=seg)
            yield p0, min(B, P - p0), self._after_fusion(k, out, cur, cur)

    @torch.no_grad()
    def localize_pairs(self, videos: "Encoded", music: "Encoded", vi, mi, pair_batch: int = 64) -> Dict[str, Optional[Tensor]]:
        """Moment localization of arbitrary (video vi[p], track mi[p]) pairs from per-item tower outputs (encode_videos /
        encode_music): per batch of pairs one made_gather_pairs, then the eval path after the towers (fusion, DETR, heads) -- no
        X-Pool, no losses.  Returns pred_logits [P, Q, 2] (None for the regression head) and pred_spans [P, Q, 2] f32."""
        c = self.cfg
        P = int(torch.as_tensor(vi).numel())
        Q = 1 if "regression" in c.mml_localization else c.num_moment_queries
        logits = None if "regression" in c.mml_localization else torch.empty(P, Q, 2, device=self.device, dtype=torch.float32)
        spans = torch.empty(P, Q, 2, device=self.device, dtype=torch.float32)
        for p0, n, out in self._localize_chunks(videos, music, vi, mi, pair_batch):
            if logits is not None:
                logits[p0:p0 + n].copy_(out["pred_logits"][:n])
            spans[p0:p0 + n].copy_(out["pred_spans"][:n])
        return dict(pred_logits=logits, pred_spans=spans)

    def _skinny(self, ws, A: Tensor, wkey: str, **kw):
        """Linear on the B*Q decoder rows: K split over workgroups so the launch fills the chip."""
        P, dws = self.P, ws["dws"]
        W = P[wkey + ".w"]
        N, K = W.shape
        slab = 64 if self.tc == torch.bfloat16 else 32
        tiles = ((A.shape[0] + 127) // 128) * ((N + 127) // 128)
        split = max(2, min(192 // max(tiles, 1), (K + slab - 1) // slab, 32, dws.numel() // (A.shape[0] * N)))
        self._linear_splitk(A, W, P[wkey + ".b"], dws, split, **kw)

    def _fused_decoder(self) -> bool:
        """The fused decoder chain (made_dec_stage) covers the scripts' configuration: bf16, one moment query, queries from the clip
        vectors (or zeros).  Everything else (f32 parity mode, Q > 1, the pooled-track query) keeps the split-K chain."""
        c = self.cfg
        # (made_dec_stage normalises whole rows of width D in its prologue: D = 256 or 512 only; other widths keep the split-K chain)
        return (self.tc == torch.bfloat16 and c.num_moment_queries == 1 and c.moment_query_type in ("video", "music", "zero", "random")
                and c.D in (256, 512) and not c.detr_pre_norm and not getattr(self, "force_unfused_decoder", False))

    def _dec_first_rows(self, ws, video: Tensor, music: Tensor) -> Tensor:
        """Raw rows feeding decoder layer 0 (reference transformer.py:73-74, model_Uni.py:216-221): the clip vectors, read in place."""
        t = self.cfg.moment_query_type
        return video if t == "video" else (music if t == "music" else ws["dzero"])

    def _dec_fused_query_side(self, ws, l: int, first_rows: Optional[Tensor]):
        """Fused chain, layer l up to the cross-attention.  Stage 1: the previous layer's norm 3 (+ the decoder output norm -> hs[l - 1]) in
        the prologue, the folded self-attention Linear + residual -> raw rows z[0].  Stage 2: norm 1 in the prologue (-> t1), + query_pos,
        the cross-attention query folded with W_k per head -> ws["dq_all"]."""
        P = self.P
        p = f"detr_transformer.decoder.layers.{l}"
        z = ws["dz"]
        if l == 0:
            ops.dec_stage(first_rows, P[p + ".sa.fold.w"], P[p + ".sa.fold.b"], z[0], res_from_x=True)
        else:
            q = f"detr_transformer.decoder.layers.{l - 1}"
            ops.dec_stage(z[2], P[p + ".sa.fold.w"], P[p + ".sa.fold.b"], z[0], ln=(P[q + ".ln3.g"], P[q + ".ln3.b"]),
                          ln2=(P["dec.norm.g"], P["dec.norm.b"]), x2_out=ws["hs"][l - 1], res_from_x=True)
        ops.dec_stage(z[0], P[p + ".ca.qk.w"], P[p + ".ca.qk.b"], ws["dq_all"], ln=(P[p + ".ln1.g"], P[p + ".ln1.b"]),
                      add=P["query_embed"], x_out=ws["t1"])

    def _decoder_queries(self, ws, video: Tensor, music: Tensor, pooled: Optional[Tensor], B: int):
        """Initial decoder queries (reference transformer.py:73-74, model_Uni.py:216-223) -> ws["tgt"]."""
        c = self.cfg
        Q, D = c.num_moment_queries, c.D
        tgt = ws["tgt"]
        if c.moment_query_type in ("video", "music"):
            src_vec = video if c.moment_query_type == "video" else music
            tgt.view(B, Q, D).copy_(src_vec[:, None, :].expand(B, Q, D))
        elif c.moment_query_type == "xpool":                             # the track's pooled vectors, averaged over the batch's videos
            src_vec = ops.masked_mean(pooled.view(B, B, D), torch.ones(B, B, device=self.device))
            tgt.view(B, Q, D).copy_(src_vec[:, None, :].expand(B, Q, D))
        else:                                                            # "zero" / "random"
            tgt.zero_()

    def _decoder_query_side(self, ws, l: int, B: int):
        """Decoder layer l up to the cross-attention: self-attention block over the queries (one folded Linear when Q = 1) ->
        ws["t1"], then the cross-attention query folded with W_k per head -> ws["dq_all"].  Reads ws["tgt"] only."""
        P = self.P
        p = f"detr_transformer.decoder.layers.{l}"
        tgt, t1 = ws["tgt"], ws["t1"]
        self._dec_self_attn(ws, l, tgt, B, R=tgt, ln1=(P[p + ".ln1.g"], P[p + ".ln1.b"]), ln1_out=t1)
        self._skinny(ws, t1, p + ".ca.qk", A2=P["query_embed"], a2_row_mod=self.cfg.num_moment_queries, out=ws["dq_all"])

    def _regression_head(self, k: "_Call", mem3: Tensor, spans_target: Optional[Tensor], with_losses: bool) -> Dict[str, Tensor]:
        """reference model/model_Uni.py:228-232,290-300: memory summed over all L positions / number of valid ones -> 3-layer
        ReLU MLP -> sigmoid; loss = 20 * L1.  The decoder's output is not used on this path, so it is not run."""
        c, P = self.cfg, self.P
        B, v_duration, out = k.B, k.v_duration, {}
        fusion = ops.masked_mean(mem3, None) / k.ws["fus_mask"].sum(dim=1, keepdim=True)   # [B, D] f32
        h1 = self._linear(fusion, P["reg_mlp.0.w"], P["reg_mlp.0.b"], act=ops.ACT_RELU)
        h2 = self._linear(h1, P["reg_mlp.1.w"], P["reg_mlp.1.b"], act=ops.ACT_RELU)
        if c.predict_center == 1:
            spans = torch.empty(B, 2, device=self.device, dtype=torch.float32)
            self._linear(h2, P["reg_mlp.2.w"], P["reg_mlp.2.b"], act=ops.ACT_SIGMOID, segs=[Seg(out=spans, ldo=2)])
            spans[:, 1] = v_duration.to(self.device, torch.float32) / c.max_m_duration
        else:
            spans = self._linear(h2, P["reg_mlp.2.w"], P["reg_mlp.2.b"], act=ops.ACT_SIGMOID, out_dtype=torch.float32)
        out["pred_spans"] = spans.view(B, 1, 2)
        if with_losses:
            tg = spans_target.to(torch.float32)
            assert tg.shape == out["pred_spans"].shape, f"spans_target.shape {tuple(tg.shape)} must equal to src_spans.shape {tuple(out['pred_spans'].shape)}"
            l1 = (out["pred_spans"] - tg).abs().mean()
            out["regression_loss_span"] = l1
            out["localization_loss"] = (l1 * 20).view(1)
        return out

    def _ca_fusion(self, ws, frame: Tensor, seg: Tensor, fm: Tensor, sm: Tensor, B: int, Tv: int, Ta: int) -> None:
        """reference model/model_Base.py:194-213 + :130-167 + :22-45 (depth 1) followed by the masked_fill of
        model/model_Uni.py:211: pre-LN cross-attention (query = segments, context = frames, 8 heads x 128, bias-free q/kv,
        kv-mask before the softmax and q-mask after it), residual, pre-LN GELU FFN with residual, final Linear -> ws["fus"]."""
        c, P = self.cfg, self.P
        D, Hc = c.D, c.ca_heads
        inner = Hc * c.ca_dim_head
        x = seg.reshape(B * Ta, D)
        nx = ops.layernorm(x, P["ca.lnq.g"], P["ca.lnq.b"], out=ws["ca_nx"])
        nc = ops.layernorm(frame.reshape(B * Tv, D), P["ca.lnc.g"], P["ca.lnc.b"], out=ws["ca_nc"])
        q = self._linear(nx, P["ca.q.w"], None, out=ws["ca_q"])
        kv = self._linear(nc, P["ca.kv.w"], None, out=ws["ca_kv"])
        kv3 = kv.view(B, Tv, 2 * inner)
        self._attention(q.view(B, Ta, inner), kv3[:, :, :inner], kv3[:, :, inner:], ws["ca_att"].view(B, Ta, inner), Hc,
                      key_mask=fm, q_mask=sm, scale=c.ca_dim_head ** -0.5)
        ax = self._linear(ws["ca_att"], P["ca.out.w"], P["ca.out.b"], R=x, out=ws["ca_x"])
        nf = ops.layernorm(ax, P["ca.lnf.g"], P["ca.lnf.b"], out=ws["ca_nx"])
        h = self._linear(nf, P["ca.ff1.w"], P["ca.ff1.b"], act=ops.ACT_GELU, out=ws["ca_h"])
        y = self._linear(h, P["ca.ff2.w"], P["ca.ff2.b"], R=ax, out=ws["ca_y"])
        self._linear(y, P["ca.final.w"], P["ca.final.b"], out_row_mask=sm.reshape(-1), out=ws["fus"].view(B * Ta, D))

    def _retrieval_loss(self, ws: Dict[str, Tensor], video: Tensor, music: Tensor, row_exclude: Optional[Tensor] = None,
                        pooled: Optional[Tensor] = None) -> None:
        """reference model/model_Uni.py:236-275 -> ws["ret_loss"]"""
        c, P = self.cfg, self.P
        rl = ws["ret_loss"]
        ls = P["logit_scale"]
        wgt = float(c.dual_single_loss_weight)
        if c.vmr_loss == "dual":
            ops.clip_loss(ws["sims_dual"], ls, rl, weight=wgt)
        elif c.vmr_loss == "single":
            ops.clip_loss(ws["sims_single"], ls, rl, weight=wgt)
        elif c.vmr_loss == "dual_single_loss_fuse":
            # row_exclude: training with --ignore_same_music 0 drops the same-track negatives of the dual loss's video -> music
            # direction (reference modules/loss.py:90-114; model_Uni.py:255)
            ops.clip_loss(ws["sims_dual"], ls, rl, weight=1.0, row_exclude=row_exclude)
            ops.clip_loss(ws["sims_single"], ls, rl, weight=1.0, accumulate=True)
        elif c.vmr_loss == "dual_single_feature_fuse":
            # reference model_Uni.py:268-273: the pooled track vectors averaged with the track's own vector, then the music-pooling
            # similarity (metrics.py:10-24) -- cos(v_n, (pooled[m, n] + music[m]) / 2); the 1/2 cancels in the cosine
            B, D = video.shape
            fused = torch.empty(B * B, D, device=self.device, dtype=torch.float32)
            ops_train.add3(fused, pooled, music[:, None, :].expand(B, B, D).contiguous())        # rows (m, n): + music[m]
            fn = ops.l2norm_rows(fused)
            vn = ops.l2norm_rows(video)
            sims = torch.empty(B, B, device=self.device, dtype=torch.float32)
            # sims[n, m] = <fn[m, n, :], vn[n, :]>: one row-vector product per video, batched over the videos
            self._linear(fn.view(B, B * D)[:, :D], vn, None, M=B, N=1, K=D, batch=B, a_z_stride=D, w_z_stride=D,     # rows m of video 0, stride B*D
                       segs=[Seg(out=sims, ldo=1, out_z_stride=B)])
            ws["sims_fused"], ws["ff_fused"], ws["ff_fn"], ws["ff_vn"] = sims, fused, fn, vn      # (the training path's backward reads them)
            ops.clip_loss(sims, ls, rl, weight=wgt)
        else:                                                            # dual_single_sim_fuse
            both = self.dual_sims(video, music, add=ws["sims_single"])
            ops.clip_loss(both, ls, rl, weight=wgt)

    def _frame_rows_linear(self, frame: Tensor, w: Tensor, b: Tensor, out: Tensor, B: int, Tv: int) -> None:
        """Linear over the frame rows of `fus` ([B, Tv, D] view with batch stride L*D): one launch per batch
        row block would waste launches, so express the view as A with rows_per_batch addressing on the OUTPUT
        side only when possible; here rows are gathered by a batched launch (grid.z = B)."""
        D = frame.shape[2]
        self._linear(frame[0], w, b, M=Tv, batch=B, a_z_stride=frame.stride(0), w_z_stride=0,
                   segs=[Seg(out=out, ldo=out.stride(0), out_z_stride=Tv * out.stride(0))])

    # ------------------------------------------------------------------ conveniences
    def loss_dict(self, out: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """criterion_losses [dec,5] -> the reference's 30-entry dict (main = last layer, `_i` = layer i)."""
        names = ["loss_span", "loss_giou", "loss_label", "class_error", "loss_contrastive_align"]
        nd = self.cfg.detr_dec_layers
        if "criterion_losses" not in out:                     # regression variant (reference model/model_Uni.py:296-300)
            return {"loss_span": out["regression_loss_span"], "loss_giou": 0, "loss_label": 0, "class_error": 0}
        L = out["criterion_losses"]
        d = {}
        for l in range(nd):
            suffix = "" if l == nd - 1 else f"_{l}"
            for k, n in enumerate(names):
                if n == "loss_contrastive_align" and not self.cfg.contrastive_align_loss:
                    continue
                if n == "loss_span" and not self.cfg.l1_loss:
                    continue
                if suffix and not self.cfg.aux_loss:
                    continue
                d[n + suffix] = L[l, k]
        return d

    def forward_numpy(self, inp: dict, with_losses: bool = True, want_pooled: bool = True) -> dict:
        """Host-facing helper for tests/smoke: numpy in, numpy out (synchronises)."""
        dev = self.device
        t = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in inp.items() if isinstance(v, np.ndarray)}
        o = self.forward(t["frame_feats"], t["segment_feats"], t["frame_masks"], t["segment_masks"], t["spans_target"],
                         with_losses=with_losses, want_pooled=want_pooled, v_duration=t.get("v_duration"))
        torch.cuda.synchronize()
        r = {k: v.float().cpu().numpy() for k, v in o.items() if isinstance(v, torch.Tensor) and v.dtype in (torch.float32, torch.bfloat16)}
        if with_losses and "regression" in self.cfg.mml_localization:
            r["loss_dict"] = {"loss_span": float(o["regression_loss_span"].cpu()), "loss_giou": 0, "loss_label": 0, "class_error": 0}
            r["retrieval_loss"] = float(o["retrieval_loss"].cpu())
            r["localization_loss"] = float(o["localization_loss"].cpu())
        elif with_losses:
            if int(o["matcher_status"].cpu()) != 0:
                raise ValueError("matrix contains invalid numeric entries")   # what SciPy raises in the reference
            nd = self.cfg.detr_dec_layers
            cnt = o["matcher_count"].cpu().numpy()
            pi, ti = o["matcher_pred_idx"].cpu().numpy(), o["matcher_tgt_idx"].cpu().numpy()
            r["matcher_indices"] = [(pi[nd - 1, b, :cnt[nd - 1, b]], ti[nd - 1, b, :cnt[nd - 1, b]]) for b in range(pi.shape[1])]
            r["matcher_indices_all"] = [[(pi[l, b, :cnt[l, b]], ti[l, b, :cnt[l, b]]) for b in range(pi.shape[1])] for l in range(nd)]
            r["loss_dict"] = {k: float(v.cpu()) for k, v in self.loss_dict(o).items()}
            r["retrieval_loss"] = float(o["retrieval_loss"].cpu())
            r["localization_loss"] = float(o["localization_loss"].cpu())
        return r
