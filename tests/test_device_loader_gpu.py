"""GPU: batches from the device-resident feature store (mgsv_amd/feature_store.py, csrc/feature_gather.hip).

made_gather_batch against integer arithmetic on the bit patterns (the widening is exact, so the comparison is on the int32 view);
DeviceLoader against the host DataLoader's batches uploaded the plain way; `--device_features 1` against `0` through both entry
points: the evaluation's metrics equal, the training step's inputs equal step by step."""
import numpy as np
import pytest
import torch

from device_loader_util import args as _args, assert_same_batch as _assert_same_batch, pack as _pack, split as _split, synthetic_csv as _synthetic_csv

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, M = 37, 11
SENTINEL, GUARD = 0x5A5A5A5A, 8                                # guard elements on both sides of every dst (32 bytes: dst stays 16-byte aligned)
COMMON = ["--mml_fusion", "concat", "--detr_enc_layers", "2", "--audio_short_cut", "0", "--max_v_frames", "20", "--max_m_duration", "100",
          "--synthetic_features", "1", "--num_workers", "0", "--batch_size_val", "16", "--save_model", "0", "--tb_writer", "0"]


def _bits16(rng, shape):
    a = rng.integers(0, 1 << 16, size=shape, dtype=np.uint16)
    a.reshape(-1)[:8] = [0x7FC1, 0xFF81, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x807F, 0x7FFF]    # NaNs with payloads, +-inf, -0, subnormals
    return a


def _bits32(rng, shape):
    a = rng.integers(0, 1 << 32, size=shape, dtype=np.uint32)
    a.reshape(-1)[:8] = [0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF]
    return a


def _sources():
    """(torch source on the device, its row map or None, the int32 patterns of the widened rows): built once, never written"""
    rng = np.random.default_rng(0)
    row = rng.integers(0, M, size=N).astype(np.int32)           # several samples share a row
    row[5], row[6] = M, -3                                      # two map entries outside [0, rows): zero rows
    out = []

    def bf16(shape, r):
        b = _bits16(rng, shape)
        out.append((torch.from_numpy(b.view(np.int16)).view(torch.bfloat16).to(DEV), r, (b.astype(np.uint32) << 16).view(np.int32)))

    def f32(shape, r):
        b = _bits32(rng, shape)
        out.append((torch.from_numpy(b.view(np.int32)).to(DEV).view(torch.float32), r, b.view(np.int32)))

    def u8(shape, r):
        b = rng.integers(0, 256, size=shape, dtype=np.uint8)
        b.reshape(-1)[:3] = [0, 255, 1]
        out.append((torch.from_numpy(b).to(DEV), r, b.astype(np.float32).view(np.int32)))

    bf16((N, 20 * 512), None); f32((M, 40 * 768), row); u8((N, 20), None); u8((M, 33), row); f32((N, 2), None); f32((N, 1), None)
    bf16((N, 7), None)
    # the f32 [M, 40 * 768] data once more as a view that starts one element into its buffer: the element path next to the 16-byte one
    src, _, want = out[1]
    shifted = torch.empty(src.numel() + 1, dtype=torch.float32, device=DEV)
    shifted[1:].view(torch.int32).copy_(src.view(torch.int32).reshape(-1))
    out.append((shifted[1:].view(M, 40 * 768), row, want))
    assert shifted[1:].data_ptr() % 16 == 4 and src.data_ptr() % 16 == 0
    return out, torch.from_numpy(row).to(DEV), row


@pytest.fixture(scope="module")
def sources():
    return _sources()


def _index(B):
    if B == 1:
        return [N - 1]
    if B == 5:
        return [0, N - 1, -1, N, 0]
    rng = np.random.default_rng(B)
    return [0, N - 1, -1, N, 5, 6, 5, 0] + [int(i) for i in rng.integers(0, N, size=B - 8)]     # 5 and 6: the bad map entries


@pytest.mark.parametrize("B", [1, 5, 64])
def test_gather_batch_moves_exact_bits_and_stays_inside_dst(sources, B):
    from mgsv_amd import ops
    arrays, row_dev, row = sources
    idx = _index(B)
    index = torch.tensor(idx, dtype=torch.int32, device=DEV)
    bufs, dsts = [], []
    for src, _, _ in arrays:
        e = src.shape[1]
        buf = torch.full((GUARD + B * e + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        bufs.append(buf)
        dsts.append(buf[GUARD:GUARD + B * e].view(torch.float32).view(B, e))
    assert len(arrays) == 8
    ops.gather_batch([(src, None if r is None else row_dev, dst) for (src, r, _), dst in zip(arrays, dsts)], index, N)
    torch.cuda.synchronize()
    for k, ((src, r, want), buf) in enumerate(zip(arrays, bufs)):
        e = src.shape[1]
        exp = np.zeros((B, e), dtype=np.int32)
        for b, s in enumerate(idx):
            if 0 <= s < N:
                rr = s if r is None else int(r[s])
                if 0 <= rr < want.shape[0]:
                    exp[b] = want[rr]
        got = buf.cpu().numpy()
        assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all(), f"array {k}: guard overwritten"
        assert np.array_equal(got[GUARD:-GUARD].reshape(B, e), exp), f"array {k}"
    # the aligned and the shifted copy of the same data: the two paths give the same bits
    assert torch.equal(bufs[1][GUARD:-GUARD], bufs[7][GUARD:-GUARD])


def test_gather_batch_refusals_are_errors_not_faults(sources):
    from mgsv_amd import _lib, ops
    arrays, row_dev, _ = sources
    index = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    src = arrays[4][0]                                          # f32 [N, 2]
    dst = [torch.zeros(2, 2, device=DEV) for _ in range(9)]
    ops.gather_batch([(src, None, d) for d in dst[:8]], index, N)            # eight arrays are accepted
    torch.cuda.synchronize()
    assert all(torch.equal(d.view(torch.int32), src[:2].view(torch.int32)) for d in dst[:8])
    with pytest.raises(_lib.MadeError, match="n_arrays=9"):
        ops.gather_batch([(src, None, d) for d in dst], index, N)
    with pytest.raises(_lib.MadeError, match="n_arrays=0"):
        ops.gather_batch([], index, N)
    with pytest.raises(_lib.MadeError, match="null src or dst"):
        ops.gather_batch([(src, None, dst[0]), (src, None, None)], index, N)
    with pytest.raises(_lib.MadeError, match="n_samples"):
        ops.gather_batch([(src, None, dst[0])], index, -1)
    ops.gather_batch([(src, None, torch.zeros(0, 2, device=DEV))], index[:0], N)                # B == 0: nothing to do
    torch.cuda.synchronize()
    assert not dst[8].any()


@pytest.mark.filterwarnings("ignore")
@pytest.mark.parametrize("source", ["pt", "f32", "bf16"])
def test_device_loader_yields_the_host_loaders_batches(tmp_path, source):
    from mgsv_amd import driver
    from mgsv_amd.feature_store import DeviceLoader
    csv, frozen = _split(tmp_path, 19, 9, odd_mask=(source == "pt"))
    if source != "pt":
        _pack(frozen, csv, source)
    common = ["--frozen_feature_path", frozen, "--max_v_frames", "20", "--max_m_duration", "100", "--train_csv", csv]
    host_args, dev_args = _args(common), _args(common + ["--device_features", "1"])
    for train in (True, False):
        torch.manual_seed(21)
        host_loader = driver.make_loader(csv, host_args, 8, train, 1, 0)[0]
        host = [[b for b in host_loader] for _ in range(2)]
        torch.manual_seed(21)
        dev_loader, n, sampler = driver.make_loader(csv, dev_args, 8, train, 1, 0)
        assert isinstance(dev_loader, DeviceLoader) and n == 19 and sampler is None and len(dev_loader) == len(host_loader)
        assert dev_loader.store.t["video_feats"].dtype == (torch.bfloat16 if source == "bf16" else torch.float32)
        for epoch in range(2):
            dev = [b for b in dev_loader]
            assert [len(m["video_id"]) for _, m, _ in dev] == ([8, 8] if train else [8, 8, 3])
            for got, want in zip(dev, host[epoch]):
                assert all(t.is_cuda for t in (*got[0].values(), got[1]["v_duration"], got[1]["m_duration"], got[1]["gt_moment"], got[2]))
                uploaded = ({k: v.to(DEV) for k, v in want[0].items()}, {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in want[1].items()},
                            want[2].to(DEV))
                for k in got[0]:
                    assert torch.equal(got[0][k], uploaded[0][k]), k
                for k in ("v_duration", "m_duration", "gt_moment"):
                    assert torch.equal(got[1][k], uploaded[1][k]), k
                assert torch.equal(got[2], uploaded[2])
                _assert_same_batch(got, want)                   # keys, dtypes, shapes, ids


@pytest.mark.parametrize("in_flight", ["2", "1"])
def test_evaluation_from_the_store_scores_the_split_identically(tmp_path, in_flight):
    from mgsv_amd import driver
    csv = str(tmp_path / "test.csv")
    _synthetic_csv(csv, 32, 2)
    base = ["--name", "df", "--test_csv", csv, "--output_dir", str(tmp_path / "logs"), "--eval_in_flight", in_flight, "--compute_dtype", "f32"] + COMMON
    host = driver.main_test(base)
    dev = driver.main_test(base + ["--device_features", "1"])
    assert dev["ret"] == host["ret"] and dev["loc"] == host["loc"] and dev["com"] == host["com"]
    assert set(dev["ret"]) >= {"R1", "R5", "R10"} and 0 <= dev["loc"]["mIoU"] <= 1


def test_training_from_the_store_feeds_the_step_the_same_batches(tmp_path, monkeypatch):
    from mgsv_amd import driver
    from mgsv_amd.trainer import MadeTrainer
    tr, va = str(tmp_path / "train.csv"), str(tmp_path / "val.csv")
    _synthetic_csv(tr, 24, 4); _synthetic_csv(va, 16, 5)
    seen = []
    step = MadeTrainer.train_step

    def recording(self, ff, sf, fm, sm, tg, *a, **kw):
        seen.append([t.clone() for t in (ff, sf, fm, sm, tg, kw["v_duration"])])
        return step(self, ff, sf, fm, sm, tg, *a, **kw)

    monkeypatch.setattr(MadeTrainer, "train_step", recording)
    runs = []
    for flag in ("0", "1"):
        seen.clear()
        res = driver.main_train(["--name", "df" + flag, "--do_train", "--epochs", "2", "--batch_size_train", "8", "--train_csv", tr, "--val_csv", va,
                                 "--output_dir", str(tmp_path / "logs"), "--compute_dtype", "f32", "--seed", "7", "--device_features", flag] + COMMON)
        assert sorted(res) == [1, 2] and np.isfinite([r["train_loss"] for r in res.values()]).all()
        runs.append(list(seen))
    assert len(runs[0]) == len(runs[1]) == 6
    for a, b in zip(*runs):
        for x, y in zip(a, b):
            assert x.is_cuda and y.is_cuda and x.dtype == y.dtype and torch.equal(x, y)
