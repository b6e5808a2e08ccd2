"""CPU: grounding without a GPU -- the grounded-recall metric on hand-built ranks and IoUs, the --ground_topk flag of both
command lines, and the argument validation of made_topk_groups / made_gather_pairs (rejected before any HIP call)."""
import os

import numpy as np
import pytest

from mgsv_amd import _lib


def _lib_built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_grounded_recall_hand_built():
    from mgsv_amd.grounding import grounded_recall
    # 4 videos, ground-truth groups 0..3; grounded lists of K = 3
    tg = np.array([[0, 5, 6],      # gt first, IoU 0.8: hit at 1 for both thresholds
                   [7, 1, 8],      # gt second, IoU 0.6: hit at 5 / 10 for 0.5 only
                   [2, 9, -1],     # gt first, IoU exactly 0.5: not > 0.5 (a tie at theta is a miss)
                   [4, 5, 6]])     # gt absent (an IoU > theta in another track does not count)
    iou = np.array([[0.8, 0.9, 0.9],
                    [0.95, 0.6, 0.1],
                    [0.5, 0.9, 0.0],
                    [0.99, 0.99, 0.99]])
    gt = np.array([0, 1, 2, 3])
    m = grounded_recall(tg, gt, iou)
    assert m == {"GR1_iou0.5": 25.0, "GR5_iou0.5": 50.0, "GR10_iou0.5": 50.0,
                 "GR1_iou0.7": 25.0, "GR5_iou0.7": 25.0, "GR10_iou0.7": 25.0}
    # a tie exactly at 0.7 is a miss at 0.7 and a hit at 0.5
    m2 = grounded_recall(np.array([[3]]), np.array([3]), np.array([[0.7]]))
    assert m2["GR1_iou0.7"] == 0.0 and m2["GR1_iou0.5"] == 100.0
    # k larger than the list (fewer groups than k): the whole list is used, -1 entries never match
    m3 = grounded_recall(np.array([[-1, 4], [2, -1]]), np.array([4, -1]), np.array([[0.9, 0.9], [0.9, 0.9]]), ks=(1, 5, 100))
    assert m3["GR1_iou0.5"] == 0.0 and m3["GR5_iou0.5"] == 50.0 and m3["GR100_iou0.5"] == 50.0


@pytest.mark.parametrize("for_test", [False, True])
def test_ground_topk_flag_on_both_command_lines(for_test):
    from mgsv_amd import driver
    a = driver.parse_option(["--name", "x"], for_test=for_test)
    assert a.ground_topk == 0
    b = driver.parse_option(["--name", "x", "--ground_topk", "5"], for_test=for_test)
    assert b.ground_topk == 5


FAKE = 4096          # a non-null "device pointer": validation rejects the call before anything reads it


def _topk(l, sims=FAKE, ld=100, gid=None, Nv=4, Nm=100, G=0, K=10, idx=FAKE, score=FAKE, ws=None, wsb=0):
    return l.made_topk_groups(sims, ld, gid, Nv, Nm, G, K, idx, score, ws, wsb, None)


def test_topk_groups_rejects_bad_arguments():
    l = _lib_built()
    bad = -1                                                        # MADE_ERR_INVALID_ARG
    assert _topk(l, K=0) == bad
    assert _topk(l, K=257) == bad
    assert _topk(l, ld=99) == bad                                   # ld < Nm
    assert _topk(l, Nm=0, ld=0) == bad
    assert _topk(l, Nv=-1) == bad
    assert _topk(l, gid=FAKE, G=32769) == bad                      # n_groups > 32768
    assert _topk(l, gid=FAKE, G=0) == bad
    assert _topk(l, sims=None) == bad
    assert _topk(l, idx=None) == bad
    assert _topk(l, score=None) == bad
    assert _topk(l, Nm=(1 << 24) + 1, ld=(1 << 24) + 1) == bad      # longer rows than the multi-block path serves
    # long rows without groups need the workspace made_topk_groups_ws_bytes names
    need = l.made_topk_groups_ws_bytes(4, 100003, 100)
    assert need > 0 and l.made_topk_groups_ws_bytes(4, 4000, 100) == 0
    assert _topk(l, Nm=100003, ld=100003, K=100) == bad
    assert _topk(l, Nm=100003, ld=100003, K=100, ws=FAKE, wsb=need - 1) == bad
    assert "workspace" in l.made_last_error().decode()


def _gather(l, **kw):
    a = dict(vi=FAKE, mi=FAKE, P=8, Nv=4, Nm=4, v_tok=FAKE, v_tok_s=30 * 256, v_mask=FAKE, v_mask_s=30, v_vec=FAKE, v_vec_s=256,
             m_tok=FAKE, m_tok_s=96 * 256, m_mask=FAKE, m_mask_s=96, m_vec=FAKE, m_vec_s=256, Tv=30, Ta=96, D=256, dtype=1,
             fo=FAKE, fo_s=126 * 256, so=FAKE, so_s=126 * 256, fmo=FAKE, smo=FAKE, vo=FAKE, mo=FAKE)
    a.update(kw)
    return l.made_gather_pairs(*a.values(), None)


def test_gather_pairs_rejects_bad_arguments():
    l = _lib_built()
    bad = -1
    for k in ("vi", "mi", "v_tok", "v_mask", "v_vec", "m_tok", "m_mask", "m_vec", "fo", "so", "fmo", "smo", "vo", "mo"):
        assert _gather(l, **{k: None}) == bad, k
    assert _gather(l, dtype=7) == bad
    assert _gather(l, P=-1) == bad
    assert _gather(l, Tv=0) == bad
    assert _gather(l, v_tok_s=29 * 256) == bad                      # item stride shorter than the item
    assert _gather(l, m_mask_s=95) == bad
    assert _gather(l, v_vec_s=255) == bad
    assert _gather(l, fo_s=29 * 256) == bad
    assert _gather(l, m_tok=FAKE + 8) == bad                        # 16-byte copies: misaligned token rows
    assert _gather(l, m_tok_s=96 * 256 + 4) == bad                  # ... or strides
    assert _gather(l, D=4, v_tok_s=120, m_tok_s=384, fo_s=504, so_s=504, v_vec_s=4, m_vec_s=4) == bad   # D * 2 bytes not a multiple of 16
