"""CPU: a MadeTrainer's forward() is MadeEngine's, and the trainer defines stage methods of its own (_detr_encoder_fwd, _decoder_fwd, _heads_fwd,
_retrieval_fwd, _dec_query_side, _index_lists, _fused_lists_fwd, _dec_fill_tgt, _dec_self_attn_fwd, ...).  An engine stage under one of the
trainer's names would be replaced silently in every trainer's inference forward.  No library, no device."""
from mgsv_amd.engine import MadeEngine
from mgsv_amd.trainer import MadeTrainer

# the schedule's tail, the stages and the helpers that the split of MadeEngine.forward / xpool_sims into stages added
ENGINE_STAGES = ["_after_fusion", "_row_lists", "_fused_lists", "_retrieval", "_detr_encoder", "_enc_layer_post_norm", "_enc_layer_pre_norm",
                 "_dec_open", "_decoder", "_dec_self_attn", "_dec_cross_attn", "_dec_layer_pre_norm", "_dec_layer_fused", "_dec_layer_splitk",
                 "_short_cut", "_music_per_query", "_heads", "_criterion", "_xpool_path", "_xpool_track_bufs", "_xpool_tracks", "_xpool_chunks"]


def test_trainer_overrides_no_engine_stage():
    missing = [n for n in ENGINE_STAGES if n not in MadeEngine.__dict__]
    assert not missing, f"not engine methods (renamed? update the list): {missing}"
    shadowed = [n for n in ENGINE_STAGES if n in MadeTrainer.__dict__]
    assert not shadowed, f"MadeTrainer replaces the engine's {shadowed} in its inherited forward()"
