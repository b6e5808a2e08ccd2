"""Grounding a set of videos in a music library: each video's best k tracks and the moment of each track to play under it.

MGSV ("Music Grounding by Short Video") asks for a track AND its moment.  The evaluation scores the two halves apart: retrieval
over the whole [N_v, N_m] similarity matrix, localization on the ground-truth (video, track) pair only.  `ground` joins them:

  1. similarities: the same vmr-loss branch the evaluation uses (`similarity_matrix`), unless the caller passes the matrix;
  2. selection: `made_topk_groups` -- the best k groups of every row (groups = music ids: a track listed twice counts once);
  3. localization: `MadeEngine.localize_pairs` on the N_v * k (video, track) pairs from the per-item tower outputs (no tower,
     no X-Pool recomputed), one workspace for all batches of pairs;
  4. moment: the top-scoring query's span in seconds (made_span_iou's `pred_out`; the regression head's one span as the
     evaluation converts it), clamped to [0, min(max_m_duration, the track's duration)].

With `windows` (mgsv_amd/windows.py) the columns of the library are overlapping windows of tracks longer than max_m_duration: a
track's score is its best window's (the same made_topk_groups, groups = the windows of a track), `made_group_topw` names the best
w windows of every selected track from the groups' CSR, localization runs on the N_v * k * w (video, window) pairs, and
`made_merge_moments` puts every query of those windows on the track's own time axis and keeps the best n after a greedy
suppression of overlapping ones -- the same passage seen through two overlapping windows is reported once.

A pair's localization depends on that pair's video and track only (every kernel after the towers computes a sample's rows
independently of the rest of the batch), so the moment found in the ground-truth track is the one the batched evaluation scores.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from .engine import Encoded, MadeEngine
from .windows import Windows, group_csr

Tensor = torch.Tensor


@dataclass
class Grounding:
    """Device tensors, [N_v, k] each: track (int32 column of the representative track, -1 past the number of groups), score
    (similarity), start / end (seconds), confidence (foreground probability of the chosen query; NaN for the regression head).
    Grounded over windows (`ground(..., windows=...)`): track is the TRACK's index, start / end / confidence are [N_v, k, n] for
    n = moments > 1 ([N_v, k] for one moment) on the track's own time axis, NaN past the moments kept, and window (int32, the shape
    of start) is the column each moment came from, -1 where there is none."""
    track: Tensor
    score: Tensor
    start: Tensor
    end: Tensor
    confidence: Tensor
    window: Optional[Tensor] = None
    windows: Optional[Windows] = None

    @property
    def k(self) -> int:
        return self.track.shape[1]

    def to_records(self, video_ids: Sequence, music_ids: Sequence) -> List[dict]:
        """One JSON-ready dict per video: {"video_id", "tracks": [{"music_id", "score", "start", "end", "confidence"}, ...]}
        (music_ids indexed by track column; entries past the number of groups are left out).  Grounded over windows, music_ids is
        indexed by track and every track holds "moments": [{"start", "end", "confidence", "window_offset"}, ...] instead of one
        start / end / confidence."""
        if self.windows is not None:
            return self._window_records(video_ids, music_ids)
        tr, sc, st, en, cf = (t.cpu().numpy() for t in (self.track, self.score, self.start, self.end, self.confidence))
        out = []
        for v, vid in enumerate(video_ids):
            ent = []
            for j in range(tr.shape[1]):
                m = int(tr[v, j])
                if m < 0:
                    continue
                c = float(cf[v, j])
                ent.append(dict(music_id=music_ids[m], score=float(sc[v, j]), start=float(st[v, j]), end=float(en[v, j]),
                                confidence=None if math.isnan(c) else c))
            out.append(dict(video_id=vid, tracks=ent))
        return out

    def _window_records(self, video_ids: Sequence, music_ids: Sequence) -> List[dict]:
        tr, sc = self.track.cpu().numpy(), self.score.cpu().numpy()
        Nv, k = tr.shape
        st, en, cf, wi = (t.cpu().numpy().reshape(Nv, k, -1) for t in (self.start, self.end, self.confidence, self.window))
        out = []
        for v, vid in enumerate(video_ids):
            ent = []
            for j in range(k):
                m = int(tr[v, j])
                if m < 0:
                    continue
                moms = []
                for i in range(st.shape[2]):
                    if wi[v, j, i] < 0:
                        continue
                    c = float(cf[v, j, i])
                    moms.append(dict(start=float(st[v, j, i]), end=float(en[v, j, i]), confidence=None if math.isnan(c) else c,
                                     window_offset=float(self.windows.offset[wi[v, j, i]])))
                ent.append(dict(music_id=music_ids[m], score=float(sc[v, j]), moments=moms))
            out.append(dict(video_id=vid, tracks=ent))
        return out


def similarity_matrix(engine: MadeEngine, video: Tensor, seg: Tensor, seg_mask: Tensor, music: Tensor) -> Tensor:
    """[N_v, N_m] f32 similarities by the configuration's vmr loss, the branch the evaluation ranks with (reference
    test-MaDe.py:386-408): cosine only for "dual" (or no X-Pool tower), X-Pool only for "single", X-Pool + cosine otherwise.
    seg [N_m, S, D] may be a strided view (the sharded retrieval's packed records)."""
    c = engine.cfg
    dev = engine.device
    video = video.to(dev, torch.float32).contiguous()
    music = music.to(dev, torch.float32).contiguous()
    seg_mask = seg_mask.to(dev, torch.float32).contiguous()
    if "XA" not in c.vmr_fusion or c.vmr_loss == "dual":
        return engine.dual_sims(video, music)
    if c.vmr_loss == "single":
        return engine.xpool_sims(video, seg.to(engine.tc), seg_mask if c.fusion_mask == 1 else None)
    return engine.retrieval_sim_matrix(video, seg.to(dev), seg_mask, music)


def _group_tensor(group_id, Nm: int, dev):
    if group_id is None:
        return None, Nm
    g = torch.as_tensor(np.asarray(group_id.cpu() if isinstance(group_id, Tensor) else group_id, dtype=np.int32))
    assert g.numel() == Nm, "group_id needs one entry per track"
    return g.to(dev).contiguous(), int(g.max()) + 1


@torch.no_grad()
def ground(engine: MadeEngine, videos: Encoded, music: Encoded, k: int, sims: Optional[Tensor] = None, group_id=None,
           pair_batch: int = 64, windows: Optional[Windows] = None, windows_per_track: int = 1, moments: int = 1,
           nms_iou: float = 0.5) -> Grounding:
    """Each video's best k tracks (groups of columns sharing a music id when group_id [N_m] is given) and the moment in each.
    windows: the columns of `music` are windows of tracks (music.duration = the windows' durations, group_id one entry per TRACK):
    each track's best `windows_per_track` windows are localized and their queries merged into up to `moments` moments per track on
    the track's time axis, a candidate being dropped when its IoU with a better one kept exceeds nms_iou."""
    c = engine.cfg
    dev = engine.device
    Nv, Nm = len(videos), len(music)
    if sims is None:
        sims = similarity_matrix(engine, videos.vec, music.tokens, music.mask, music.vec)
    sims = sims.to(dev, torch.float32)
    if sims.stride(1) != 1:
        sims = sims.contiguous()
    if windows is not None:
        return _ground_windows(engine, videos, music, k, sims, group_id, pair_batch, windows, int(windows_per_track), int(moments),
                               float(nms_iou))
    gid, G = _group_tensor(group_id, Nm, dev)
    kk = max(1, min(int(k), G))
    track, score = ops.topk_groups(sims, kk, gid, G)
    P = Nv * kk
    vi = torch.arange(Nv, device=dev, dtype=torch.int32).repeat_interleave(kk)
    mi = track.reshape(-1)
    mi = torch.where(mi < 0, torch.zeros_like(mi), mi)             # (no track: localized against track 0, reported as -1 / NaN)
    pred = torch.empty(P, 3, device=dev, dtype=torch.float32)      # start, end (seconds, unclamped), confidence
    regression = "regression" in c.mml_localization
    mx = float(c.max_m_duration)
    scratch = None
    for p0, n, out in engine._localize_chunks(videos, music, vi, mi, pair_batch):
        if regression:                                             # the one regressed span (driver._batch_iou's conversion)
            sp = out["pred_spans"][:n, 0]
            pred[p0:p0 + n, 0] = (sp[:, 0] - 0.5 * sp[:, 1]) * mx
            pred[p0:p0 + n, 1] = (sp[:, 0] + 0.5 * sp[:, 1]) * mx
            pred[p0:p0 + n, 2] = float("nan")
            continue
        B, Q = out["pred_logits"].shape[0], out["pred_logits"].shape[1]
        if scratch is None:                                        # made_span_iou's IoU inputs / output (unused here)
            scratch = (torch.zeros(B, 2, device=dev), torch.ones(B, device=dev), torch.empty(B, device=dev))
        _lib.check(_lib.lib().made_span_iou(out["pred_logits"].data_ptr(), out["pred_spans"].data_ptr(), scratch[0].data_ptr(),
                                            scratch[1].data_ptr(), n, Q, int(c.foreground_label), mx, scratch[2].data_ptr(),
                                            pred[p0:p0 + n].data_ptr(), torch.cuda.current_stream().cuda_stream), "made_span_iou")
    hi = torch.full((P,), mx, device=dev, dtype=torch.float32)
    if music.duration is not None:
        hi = torch.minimum(hi, music.duration.to(dev, torch.float32)[mi.long()])
    start = torch.minimum(pred[:, 0].clamp(min=0), hi)
    end = torch.minimum(pred[:, 1].clamp(min=0), hi)
    conf = pred[:, 2].clone()
    none = track.reshape(-1) < 0
    if bool(none.any()):
        nan = torch.full_like(start, float("nan"))
        start, end, conf = torch.where(none, nan, start), torch.where(none, nan, end), torch.where(none, nan, conf)
    return Grounding(track=track, score=score, start=start.view(Nv, kk), end=end.view(Nv, kk), confidence=conf.view(Nv, kk))


def _pair_candidates(engine: MadeEngine, videos: Encoded, music: Encoded, vi: Tensor, mi: Tensor, pair_batch: int) -> Tensor:
    """[P, Q, 3] f32: every query's (start, end, foreground probability) of the pairs, seconds on the column's own axis, unclamped --
    the arithmetic of `ground` without windows: made_span_iou's pred_out with every query a row of its own (so the top query of a
    pair is bit for bit what made_span_iou picks over the pair's Q queries); the regression head's one span, probability NaN."""
    c = engine.cfg
    dev = engine.device
    mx = float(c.max_m_duration)
    P = vi.numel()
    if "regression" in c.mml_localization:
        cand = torch.empty(P, 1, 3, device=dev, dtype=torch.float32)
        for p0, n, out in engine._localize_chunks(videos, music, vi, mi, pair_batch):
            sp = out["pred_spans"][:n, 0]
            cand[p0:p0 + n, 0, 0] = (sp[:, 0] - 0.5 * sp[:, 1]) * mx
            cand[p0:p0 + n, 0, 1] = (sp[:, 0] + 0.5 * sp[:, 1]) * mx
            cand[p0:p0 + n, 0, 2] = float("nan")
        return cand
    Q = int(c.num_moment_queries)
    cand = torch.empty(P, Q, 3, device=dev, dtype=torch.float32)
    scratch = None
    for p0, n, out in engine._localize_chunks(videos, music, vi, mi, pair_batch):
        R = out["pred_logits"].shape[0] * Q
        if scratch is None:                                        # made_span_iou's IoU inputs / output (unused here)
            scratch = (torch.zeros(R, 2, device=dev), torch.ones(R, device=dev), torch.empty(R, device=dev))
        _lib.check(_lib.lib().made_span_iou(out["pred_logits"].data_ptr(), out["pred_spans"].data_ptr(), scratch[0].data_ptr(),
                                            scratch[1].data_ptr(), n * Q, 1, int(c.foreground_label), mx, scratch[2].data_ptr(),
                                            cand[p0:p0 + n].data_ptr(), torch.cuda.current_stream().cuda_stream), "made_span_iou")
    return cand


def _ground_windows(engine: MadeEngine, videos: Encoded, music: Encoded, k: int, sims: Tensor, group_id, pair_batch: int,
                    windows: Windows, w: int, n: int, nms_iou: float) -> Grounding:
    c = engine.cfg
    dev = engine.device
    Nv, Nm = len(videos), len(music)
    if len(windows) != Nm:
        raise ValueError(f"windows describes {len(windows)} columns, the library has {Nm}")
    if not 1 <= w <= 16:
        raise ValueError(f"windows_per_track = {w}: must lie in [1, 16]")
    if n < 1:
        raise ValueError(f"moments = {n}: must be >= 1")
    if group_id is None:
        col_group, G = windows.track.astype(np.int32), windows.n_tracks
    else:
        g = np.asarray(group_id.cpu() if isinstance(group_id, Tensor) else group_id, dtype=np.int32).reshape(-1)
        if g.size != windows.n_tracks:
            raise ValueError("with windows, group_id needs one entry per track")
        col_group, G = g[windows.track], int(g.max()) + 1
    start, cols = group_csr(col_group, G)
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gid = as_dev(col_group)
    kk = max(1, min(int(k), G))
    rep, score = ops.topk_groups(sims, kk, gid, G)                 # a track's score: its best window's similarity
    wcol, wscore = ops.group_topw(sims, rep, gid, as_dev(start), as_dev(cols), w)
    vi = torch.arange(Nv, device=dev, dtype=torch.int32).repeat_interleave(kk * w)
    mi = wcol.reshape(-1)
    mi = torch.where(mi < 0, torch.zeros_like(mi), mi)             # (no window: localized against column 0, left out by the merge)
    cand = _pair_candidates(engine, videos, music, vi, mi, pair_batch)
    Q = cand.shape[1]
    duration = music.duration.to(dev, torch.float32).contiguous() if music.duration is not None else None
    st, en, cf, wi = ops.merge_moments(cand.view(Nv * kk, w, Q, 3), wcol.view(Nv * kk, w), wscore.view(Nv * kk, w), as_dev(windows.offset),
                                       duration, float(c.max_m_duration), nms_iou, n, use_prob="regression" not in c.mml_localization)
    track = torch.where(rep < 0, rep, as_dev(windows.track)[rep.clamp(min=0).long()])
    shape = (Nv, kk) if n == 1 else (Nv, kk, n)
    return Grounding(track=track, score=score, start=st.view(shape), end=en.view(shape), confidence=cf.view(shape), window=wi.view(shape),
                     windows=windows)


def moment_iou(start: Tensor, end: Tensor, gt_moment: Tensor, m_duration: Tensor, max_m_duration: float) -> Tensor:
    """IoU of predicted moments [N_v, k] (seconds) with each video's ground-truth moment [N_v, 2] in a track of m_duration [N_v]
    seconds: the evaluation's clamps (made_span_iou_se, reference music_detr/span_utils.py:119-170)."""
    Nv, k = start.shape
    dev = start.device
    pred = torch.stack([start, end], dim=-1).reshape(Nv * k, 2).to(torch.float32).contiguous()
    gt = gt_moment.to(dev, torch.float32).reshape(Nv, -1)[:, :2].repeat_interleave(k, dim=0).contiguous()
    dur = m_duration.to(dev, torch.float32).reshape(Nv).repeat_interleave(k).contiguous()
    iou = torch.empty(Nv * k, device=dev, dtype=torch.float32)
    _lib.check(_lib.lib().made_span_iou_se(pred.data_ptr(), gt.data_ptr(), dur.data_ptr(), Nv * k, float(max_m_duration), 1, 0,
                                           iou.data_ptr(), torch.cuda.current_stream().cuda_stream), "made_span_iou_se")
    return torch.nan_to_num(iou, nan=0.0).view(Nv, k)


def grounded_recall(track_groups, gt_groups, ious, ks: Sequence[int] = (1, 5, 10), thetas: Sequence[float] = (0.5, 0.7)) -> Dict[str, float]:
    """GR{k}_iou{theta}: the percentage of videos for which one of the first k grounded tracks is the ground-truth track (same group)
    AND the moment predicted in that track has IoU > theta with the ground-truth moment.  track_groups [N_v, K] (group of every
    grounded track, -1 = none), gt_groups [N_v], ious [N_v, K]; k beyond K uses all K."""
    tg = np.asarray(track_groups, dtype=np.int64)
    gt = np.asarray(gt_groups, dtype=np.int64).reshape(-1)
    iou = np.asarray(ious, dtype=np.float64)
    assert tg.ndim == 2 and tg.shape == iou.shape and tg.shape[0] == gt.shape[0]
    n = max(tg.shape[0], 1)
    hit_track = (tg == gt[:, None]) & (tg >= 0)
    out = {}
    for th in thetas:
        for k in ks:
            hit = (hit_track[:, :k] & (iou[:, :k] > th)).any(axis=1)
            out[f"GR{k}_iou{th}"] = float(hit.sum()) * 100 / n
    return out
