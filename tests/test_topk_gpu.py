"""GPU: made_topk_groups (each row's best K groups of columns) against a numpy restatement -- exact agreement, ties, NaN / inf,
strided rows, the multi-block path of long rows -- and its consistency with made_recall_ranks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def ref_topk(x: np.ndarray, K: int, gid=None):
    """numpy restatement: columns in np.argsort(-x, kind="stable") order (score descending, NaN last, lowest column first among
    equal scores); a group enters at its first column in that order (its maximum, lowest column attaining it)."""
    Nv, Nm = x.shape
    gid = np.arange(Nm) if gid is None else np.asarray(gid)
    idx = np.full((Nv, K), -1, dtype=np.int64)
    sc = np.full((Nv, K), -np.inf, dtype=np.float32)
    for r in range(Nv):
        order = np.argsort(-x[r], kind="stable")
        _, first = np.unique(gid[order], return_index=True)
        reps = order[np.sort(first)][:K]
        idx[r, :len(reps)] = reps
        sc[r, :len(reps)] = x[r, reps]
    return idx, sc


def run(x: np.ndarray, K: int, gid=None, ld=None):
    from mgsv_amd import ops
    Nv, Nm = x.shape
    if ld is not None and ld > Nm:
        full = torch.full((Nv, ld), 7.0, dtype=torch.float32)          # the padding columns hold values that would win
        full[:, :Nm] = torch.from_numpy(x)
        sims = full.cuda()[:, :Nm]
    else:
        sims = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    g = torch.from_numpy(np.asarray(gid, dtype=np.int32)).cuda() if gid is not None else None
    idx, sc = ops.topk_groups(sims, K, g, None if gid is None else int(np.max(gid)) + 1)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy()


def check(x, K, gid=None, ld=None):
    gi, gs = run(x, K, gid, ld)
    ri, rs = ref_topk(x, K, gid)
    bad = np.argwhere(gi != ri)
    assert bad.size == 0, (bad[:5], gi[tuple(bad[0])], ri[tuple(bad[0])])
    assert np.array_equal(gs, rs, equal_nan=True)


@pytest.mark.parametrize("Nv,Nm,K", [(7, 1000, 10), (3, 4000, 100), (5, 300, 256), (2, 32768, 256), (4, 17, 1)])
def test_random_rows(Nv, Nm, K):
    rng = np.random.default_rng(Nm + K)
    check(rng.standard_normal((Nv, Nm)).astype(np.float32), K)


@pytest.mark.parametrize("levels", [1, 3, 40])
def test_ties_from_quantised_rows(levels):
    rng = np.random.default_rng(levels)
    x = rng.integers(-levels // 2, levels - levels // 2, size=(6, 2000)).astype(np.float32) * 0.25     # includes -0.0 / +0.0 collisions
    x[0, ::3] = -0.0
    check(x, 50)
    check(x, 256)
    check(x, 20, gid=rng.integers(0, 300, size=2000))


def test_nan_and_infinities():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((5, 700)).astype(np.float32)
    x[0, rng.choice(700, 40, replace=False)] = np.nan
    x[1, rng.choice(700, 10, replace=False)] = np.inf
    x[1, rng.choice(700, 10, replace=False)] = -np.inf
    x[2, :] = np.nan                                                    # a row of NaN: lowest columns first
    x[3, :] = -np.inf
    x[3, 600:] = np.nan
    x[4, ::2] = np.nan
    x[4, 1::2] = np.inf
    check(x, 30)
    check(x, 30, gid=np.arange(700) % 64)


def test_strided_rows_and_single_row():
    rng = np.random.default_rng(6)
    check(rng.standard_normal((4, 999)).astype(np.float32), 33, ld=1024)
    check(rng.standard_normal((1, 5000)).astype(np.float32), 100)
    check(rng.standard_normal((1, 5000)).astype(np.float32), 100, gid=rng.integers(0, 700, size=5000))


@pytest.mark.parametrize("K", [1, 100, 256])
def test_long_rows_multi_block_path(K):
    rng = np.random.default_rng(K)
    x = rng.standard_normal((3, 100003)).astype(np.float32)
    check(x, K)
    q = np.round(x * 2).astype(np.float32)                              # ties across the 32768-column blocks
    check(q, K)


def test_groups_4000_columns_1000_groups_and_k_above_the_group_count():
    rng = np.random.default_rng(8)
    x = rng.standard_normal((9, 4000)).astype(np.float32)
    gid = rng.integers(0, 1000, size=4000)
    gid[:1000] = np.arange(1000)                                        # every group present
    check(x, 100, gid=gid)
    small = rng.integers(0, 37, size=4000)
    small[:37] = np.arange(37)
    gi, gs = run(x, 64, small)
    assert (gi[:, 37:] == -1).all() and np.isneginf(gs[:, 37:]).all()
    check(x, 64, gid=small)
    check(x[:, :50], 80)                                                # K above the number of columns


def test_first_entry_and_ranks_agree_with_recall_ranks():
    from mgsv_amd.utils.util_test import recall_ranks_device
    rng = np.random.default_rng(9)
    Nv, Nm, G, K = 64, 3000, 800, 40
    x = rng.standard_normal((Nv, Nm)).astype(np.float32)                 # continuous: tie-free
    gid = rng.integers(0, G, size=Nm)
    gid[:G] = np.arange(G)
    gt = rng.integers(0, G, size=Nv)
    sims = torch.from_numpy(x).cuda()
    rank, top1 = recall_ranks_device(sims, gid.tolist(), gt.tolist())
    rank, top1 = rank.cpu().numpy(), top1.cpu().numpy()
    gi, _ = run(x, K, gid)
    assert np.array_equal(gi[:, 0], top1)
    pos_groups = np.where(gi >= 0, gid[np.maximum(gi, 0)], -1)
    for r in range(Nv):
        where = np.flatnonzero(pos_groups[r] == gt[r])
        if rank[r] < K:
            assert where.tolist() == [rank[r]], (r, rank[r], where)
        else:
            assert where.size == 0
    q = np.round(x * 3).astype(np.float32)                               # with ties the first entry is still top1
    _, top1q = recall_ranks_device(torch.from_numpy(q).cuda(), gid.tolist(), gt.tolist())
    assert np.array_equal(run(q, K, gid)[0][:, 0], top1q.cpu().numpy())
    assert np.array_equal(run(q, K)[0][:, 0], top1q.cpu().numpy())


def test_full_size_sampled_rows():
    from mgsv_amd import ops
    g = torch.Generator(device="cuda").manual_seed(11)
    sims = torch.randn(53000, 4000, device="cuda", generator=g)
    gid = torch.randint(0, 4000, (4000,), device="cuda", generator=g, dtype=torch.int32)
    for groups in (None, gid):
        idx, sc = ops.topk_groups(sims, 100, groups, None if groups is None else 4000)
        torch.cuda.synchronize()
        rows = np.random.default_rng(12).choice(53000, 48, replace=False)
        x = sims[torch.from_numpy(rows).cuda()].cpu().numpy()
        ri, rs = ref_topk(x, 100, None if groups is None else gid.cpu().numpy())
        assert np.array_equal(idx.cpu().numpy()[rows], ri)
        assert np.array_equal(sc.cpu().numpy()[rows], rs)
