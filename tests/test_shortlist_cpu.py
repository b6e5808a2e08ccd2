"""CPU: grounding with a cosine shortlist -- the numpy restatement of the selection on a candidate list against the brute force on
the dense row (tests/filter_ref.py's masked selection), the builder of the (column -> videos) CSR that the pair kernel walks, and
the refusals that need no device."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import filter_ref as FR
import shortlist_ref as SR
from mgsv_amd.config import cfg_native
from mgsv_amd.grounding import Constraints, check_shortlist, ground, ground_library, pair_csr


def _groups(rng, N, n_groups):
    """uneven groups: a few large ones, many of one column"""
    g = rng.integers(0, n_groups, N).astype(np.int32)
    g[: N // 4] = 0                                                 # one group larger than any w
    return g


def _rows(rng, Nv, N, R, values):
    """candidate rows with ties everywhere (few distinct values), NaN, -inf, +-0; rows of 0, 1 and 2 candidates"""
    col = np.full((Nv, R), -1, np.int32)
    score = np.full((Nv, R), np.nan, np.float32)
    for r in range(Nv):
        n = [R, 0, 1, min(2, R)][r] if r < 4 else int(rng.integers(0, R + 1))
        c = rng.choice(N, size=min(n, N), replace=False)
        pos = rng.permutation(R)[:len(c)]                           # (candidates need not be packed to the front)
        col[r, pos] = c
        score[r, pos] = rng.choice(values, len(c))
    return col, score


VALUES = np.array([-np.inf, -1.0, -0.0, 0.0, 0.5, 0.5, 1.0, np.nan], np.float32)


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("R,K,w", [(1, 1, 1), (7, 3, 2), (7, 10, 3), (40, 10, 1), (256, 5, 16), (256, 256, 3)])
def test_restatement_is_the_dense_row_selection(R, K, w, grouped):
    rng = np.random.default_rng(1000 * R + 10 * K + w + grouped)
    N, Nv = 300, 9
    col_group = _groups(rng, N, 25) if grouped else None            # 25 groups: fewer than K = 256, more than K = 3
    if not grouped:
        w = 1
    cand_col, cand_score = _rows(rng, Nv, N, R, VALUES)
    got = SR.select_candidates(cand_col, cand_score, col_group, K, w)
    want = SR.dense_row_selection(cand_col, cand_score, col_group, N, K, w)
    assert FR.same(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    assert FR.same(got[1], want[1])
    assert (got[0][1] == -1).all() and np.isneginf(got[1][1]).all()             # the row without candidates
    if grouped and R >= 40:
        assert ((got[0][0] >= 0).sum(axis=1) == w).any()                        # a group larger than w filled every window slot
        assert (got[0][0][:, 0] >= 0).sum() <= 25


def test_restatement_orders_nan_lowest_and_signed_zeros_equal():
    cand_col = np.array([[5, 2, 9, 7, 3, -1]], np.int32)
    cand_score = np.array([[np.nan, -0.0, 0.0, -np.inf, 1.0, 9.0]], np.float32)
    col, score = SR.select_candidates(cand_col, cand_score, None, 6, 1)
    assert col[0, :, 0].tolist() == [3, 2, 9, 7, 5, -1]                          # 1.0, then +-0 by column, -inf, NaN, nothing
    assert np.signbit(score[0, 1:3, 0]).tolist() == [False, False] and np.isnan(score[0, 4, 0]) and np.isneginf(score[0, 5, 0])
    g = np.array([0, 0, 0, 1, 0, 1, 0, 1, 0, 1], np.int32)           # group 1: columns 3 (1.0), 9 (0.0), 7 (-inf), 5 (NaN); group 0: column 2 (-0.0)
    col, score = SR.select_candidates(cand_col, cand_score, g, 3, 2)
    assert col[0].tolist() == [[3, 9], [2, -1], [-1, -1]]           # the group's best two; one candidate, one empty window; no third group


def test_shortlist_columns_respects_eligibility_and_order():
    cos = np.array([[0.5, 0.9, 0.9, np.nan, -0.0, 0.0]], np.float32)
    elig = np.array([[True, True, True, True, True, False]])
    col, val = SR.shortlist_columns(cos, elig, 6)
    assert col[0].tolist() == [1, 2, 0, 4, 3, -1] and np.isneginf(val[0, 5]) and np.isnan(val[0, 4])
    col, _ = SR.shortlist_columns(cos, None, 2)
    assert col[0].tolist() == [1, 2]


def test_pair_csr_hand_cases():
    T = lambda a: torch.tensor(a, dtype=torch.int32)
    # three videos, R = 3: column 4 listed by all videos, column 9 by one, columns 5 .. 8 by nobody (no empty range is emitted)
    cand = T([[4, 9, -1], [-1, 4, 2], [2, -1, 4]])
    cols, start, video, slot = pair_csr(cand)
    assert cols.tolist() == [2, 4, 9] and start.tolist() == [0, 2, 5, 6]
    assert video.tolist() == [1, 2, 0, 1, 2, 0]                     # ascending inside every column
    assert slot.tolist() == [5, 6, 0, 4, 8, 1] and torch.equal(cand.reshape(-1)[slot].long(), torch.repeat_interleave(cols, torch.diff(start).long()))
    assert cols.dtype == torch.int64 and start.dtype == torch.int32 and video.dtype == torch.int32 and slot.dtype == torch.int64
    # one video
    cols, start, video, slot = pair_csr(T([[7, 3, 5]]))
    assert cols.tolist() == [3, 5, 7] and start.tolist() == [0, 1, 2, 3] and video.tolist() == [0, 0, 0] and slot.tolist() == [1, 2, 0]
    # nothing listed at all
    cols, start, video, slot = pair_csr(torch.full((4, 2), -1, dtype=torch.int32))
    assert len(cols) == 0 and start.tolist() == [0] and len(video) == 0 and len(slot) == 0
    # every video lists the same single column
    cols, start, video, _ = pair_csr(torch.full((5, 1), 11, dtype=torch.int32))
    assert cols.tolist() == [11] and start.tolist() == [0, 5] and video.tolist() == [0, 1, 2, 3, 4]
    # a random table against a plain sort of its (column, video) pairs
    rng = np.random.default_rng(4)
    tab = rng.integers(-1, 50, size=(13, 9)).astype(np.int32)
    cols, start, video, slot = pair_csr(torch.from_numpy(tab))
    pairs = sorted((int(c), i) for i in range(13) for c in tab[i] if c >= 0)
    got = list(zip(torch.repeat_interleave(cols, torch.diff(start).long()).tolist(), video.tolist()))
    assert got == pairs and tab.reshape(-1)[slot.numpy()].tolist() == [c for c, _ in pairs]


def test_refusals_without_a_device():
    cfg = cfg_native()
    assert check_shortlist(cfg, None, True) is None and check_shortlist(cfg, 256, False) == 256 and check_shortlist(cfg, 1, False) == 1
    for bad in (0, 257, -3, 2.5):
        with pytest.raises(ValueError, match="shortlist"):
            check_shortlist(cfg, bad, False)
    with pytest.raises(ValueError, match="sims"):
        check_shortlist(cfg, 8, True)
    single = cfg_native(); single.vmr_loss = "single"
    with pytest.raises(ValueError, match="no cosine term"):
        check_shortlist(single, 8, False)
    dual = cfg_native(); dual.vmr_loss = "dual"
    with pytest.raises(ValueError, match="cosine alone"):
        check_shortlist(dual, 8, False)
    no_tower = cfg_native(); no_tower.vmr_fusion = "none"
    with pytest.raises(ValueError, match="cosine alone"):
        check_shortlist(no_tower, 8, False)
    # the entry points refuse before they touch a device
    eng = SimpleNamespace(cfg=cfg, device="cpu")
    with pytest.raises(ValueError, match="sims"):
        ground(eng, [0] * 3, [0] * 5, 2, sims=np.zeros((3, 5), np.float32), shortlist=4)
    with pytest.raises(ValueError, match="shortlist"):
        ground(eng, [0] * 3, [0] * 5, 2, shortlist=300)
    with pytest.raises(ValueError, match="sims"):
        ground_library(eng, [0] * 3, None, 2, sims_fn=lambda *a: None, shortlist=4)
    with pytest.raises(ValueError, match="no cosine term"):
        ground_library(SimpleNamespace(cfg=single, device="cpu"), [0] * 3, None, 2, shortlist=4, constraints=Constraints())
