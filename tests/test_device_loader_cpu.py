"""CPU: the device-resident feature store without a device (mgsv_amd/feature_store.py DeviceFeatureStore / DeviceLoader).

A CPU store keeps the same tables and serves batches through `gather_reference` (torch indexing): its batches must equal the
collated batches of the host DataLoader in the same order, and leave torch's default generator where the host loader leaves it."""
import os

import pytest
import torch

from device_loader_util import args as _args, assert_same_batch as _assert_same_batch, pack as _pack, split as _split, synthetic_csv as _synthetic_csv


@pytest.mark.filterwarnings("ignore")
@pytest.mark.parametrize("train,world,rank", [(True, 1, 0), (False, 1, 0), (True, 2, 0), (True, 2, 1), (False, 2, 0), (False, 2, 1)])
def test_batch_order_and_generator_state_match_the_host_loader(tmp_path, train, world, rank):
    from mgsv_amd import driver
    from mgsv_amd.feature_store import DeviceLoader
    csv = str(tmp_path / "s.csv")
    _synthetic_csv(csv, 19, 3)
    common = ["--synthetic_features", "1", "--max_v_frames", "6", "--max_m_duration", "20", "--train_csv", csv]
    host_args, dev_args = _args(common), _args(common + ["--device_features", "1"])
    assert host_args.device_features == 0 and dev_args.device_features == 1
    runs = []
    for args in (host_args, dev_args):
        torch.manual_seed(1234)
        loader, n, sampler = driver.make_loader(csv, args, 4 * world, train, world, rank, device="cpu")
        assert n == 19 and (sampler is not None) == (world > 1)
        ids = []
        for epoch in (1, 2):
            if sampler is not None:
                sampler.set_epoch(epoch)
            ids.append([(tuple(m["video_id"]), tuple(m["music_id"])) for _, m, _ in loader])
            assert len(ids[-1]) == len(loader)
        runs.append((type(loader), ids, torch.get_rng_state()))
    assert runs[1][0] is DeviceLoader and runs[0][0] is torch.utils.data.DataLoader
    assert runs[0][1] == runs[1][1]
    assert torch.equal(runs[0][2], runs[1][2])
    if train:
        assert runs[0][1][0] != runs[0][1][1] and all(len(v) == 4 for e in runs[0][1] for v, _ in e)      # reshuffled; drop_last
    elif world == 1:
        assert [len(v) for v, _ in runs[0][1][0]] == [4, 4, 4, 4, 3]


@pytest.mark.filterwarnings("ignore")
@pytest.mark.parametrize("source", ["pt", "f32", "bf16"])
def test_reference_batches_equal_the_collated_batches(tmp_path, source):
    from mgsv_amd import driver
    from mgsv_amd.feature_store import DeviceFeatureStore
    csv, frozen = _split(tmp_path, 16, 7, odd_mask=(source == "pt"))
    if source != "pt":
        _pack(frozen, csv, source)
    common = ["--frozen_feature_path", frozen, "--max_v_frames", "20", "--max_m_duration", "100", "--train_csv", csv]
    host_args, dev_args = _args(common), _args(common + ["--device_features", "1"])
    ds = driver.MGSV_EC_Dataset(csv, host_args)
    store = DeviceFeatureStore.from_dataset(ds, "cpu")
    assert len(store) == 16 and store.t["music_feats"].shape[0] == len(set(store.music_ids)) <= 8 and store.t["video_feats"].shape[0] == 16
    want_f = torch.bfloat16 if source == "bf16" else torch.float32
    want_m = torch.float32 if source == "pt" else torch.uint8
    assert store.t["video_feats"].dtype == store.t["music_feats"].dtype == want_f
    assert store.t["video_mask"].dtype == store.t["music_mask"].dtype == want_m
    if source == "pt":
        assert any(float(v) not in (0.0, 1.0) for v in store.t["video_mask"].flatten()) and (store.t["music_mask"] == 2.0).any()
    with pytest.raises(RuntimeError):
        store.gather(torch.zeros(2, dtype=torch.int32))         # a CPU store cannot launch, and does not pretend to
    for train in (True, False):
        torch.manual_seed(5)
        host = [b for b in driver.make_loader(csv, host_args, 5, train, 1, 0)[0]]
        torch.manual_seed(5)
        dev = [b for b in driver.make_loader(csv, dev_args, 5, train, 1, 0, device="cpu")[0]]
        assert len(host) == len(dev) == (3 if train else 4)
        for got, want in zip(dev, host):
            _assert_same_batch(got, want)
    # the gather's rule for numbers outside the split: a zero row, like made_gather_rows
    d, m, s = store.gather_reference([3, -1, 16, 3])
    assert torch.equal(d["frame_feats"][0], d["frame_feats"][3]) and d["frame_feats"][0].abs().sum() > 0
    for t in (*d.values(), m["v_duration"], m["gt_moment"], s):
        assert not t[1].any() and not t[2].any()


def test_a_store_past_the_limit_is_refused(tmp_path):
    from mgsv_amd import driver
    from mgsv_amd.feature_store import DeviceFeatureStore
    csv = str(tmp_path / "s.csv")
    _synthetic_csv(csv, 19, 3)
    args = _args(["--synthetic_features", "1", "--max_v_frames", "6", "--max_m_duration", "20"])
    ds = driver.MGSV_EC_Dataset(csv, args)
    store = DeviceFeatureStore.from_dataset(ds, "cpu")
    need = store.nbytes
    assert need > 19 * 6 * 512 * 4
    assert DeviceFeatureStore.from_dataset(ds, "cpu", limit_bytes=need).nbytes == need
    with pytest.raises(ValueError) as e:
        DeviceFeatureStore.from_dataset(ds, "cpu", limit_bytes=need - 1)
    assert str(need) in str(e.value) and str(need - 1) in str(e.value)


def test_getitem_is_unchanged_by_its_split_into_two_parts(tmp_path):
    import pandas as pd
    from mgsv_amd import driver
    csv, frozen = _split(tmp_path, 6, 11)
    df = pd.read_csv(csv)
    df.loc[2, "music_end"] = 150.0                               # past max_m_duration: the clamp reaches gt_moment too
    df.to_csv(csv, index=False)
    args = _args(["--frozen_feature_path", frozen, "--max_v_frames", "20", "--max_m_duration", "100"])
    ds = driver.MGSV_EC_Dataset(csv, args)
    for i in range(6):
        r = df.iloc[i]
        data, meta, spans = ds[i]
        vid, mid = str(r["video_id"]), str(r["music_id"])
        st, en = float(r["music_start"]), float(r["music_end"])
        gt = torch.tensor([[st, en]])
        gt[:, 1] = torch.clamp(gt[:, 1], max=100)
        want_spans = torch.stack([(gt[:, 0] + gt[:, 1]) / 2.0 / 100, (gt[:, 1] - gt[:, 0]) / 100], dim=-1)
        assert meta["video_id"] == vid and meta["music_id"] == mid
        assert torch.equal(meta["v_duration"], torch.tensor(float(r["video_end"]) - float(r["video_start"])))
        assert torch.equal(meta["m_duration"], torch.tensor(float(r["music_total_duration"])))
        assert torch.equal(meta["gt_moment"], gt) and meta["gt_moment"].shape == (1, 2)
        assert torch.equal(spans, want_spans) and spans.shape == (1, 2)
        for key, sub, kind, ident in (("frame", "vit_feature1", "vit", vid), ("segment", "ast_feature2p5", "ast", mid)):
            f = torch.load(os.path.join(frozen, sub, f"{kind}_feature", f"{ident}.pt"))
            m = torch.load(os.path.join(frozen, sub, f"{kind}_mask", f"{ident}.pt"))
            assert torch.equal(data[f"{key}_mask"], m.float())
            assert torch.equal(data[f"{key}_feats"], f.masked_fill(m.unsqueeze(-1) == 0, 0).float())
    assert float(ds[2][1]["gt_moment"][0, 1]) == 100.0


class _Canned:
    """A model whose fused train step returns canned tensors: train_one_epoch's bookkeeping alone."""

    def __init__(self, steps, reads):
        self.steps, self.k, self._train_seed = steps, 0, 0
        self.reads, self.reads_at = reads, []
        self.criterion = type("C", (), {"foreground_label": 0})()

    def train(self):
        pass

    def _trainer_ready(self):
        return self

    def train_step(self, ff, *a, **kw):
        o = self.steps[self.k]
        self.k += 1
        self.reads_at.append(self.reads[0])
        return {"retrieval_loss": o["ret"], "localization_loss": o["loc"], "pred_spans": o["spans"]}


def test_deferred_reads_log_and_return_the_per_step_numbers(tmp_path, monkeypatch):
    """train_one_epoch reads nothing back per step; what it logs at the display points and returns is what the per-step formula
    (meter += float(x) * b after every step, IoUs extended per step) gives."""
    import logging
    from mgsv_amd import driver
    from mgsv_amd.utils.util_test import IoU_metrics
    g = torch.Generator().manual_seed(0)
    n_steps, sizes = 7, [4, 4, 4, 4, 4, 4, 3]
    steps, batches = [], []
    for b in sizes:
        c, w = torch.rand(b, generator=g) * 0.6 + 0.2, torch.rand(b, generator=g) * 0.3 + 0.05
        steps.append({"ret": torch.rand(1, generator=g) * 3, "loc": torch.rand(1, generator=g) * 7, "spans": torch.stack([c, w], -1).reshape(b, 1, 2)})
        st = torch.rand(b, generator=g) * 50
        meta = {"gt_moment": torch.stack([st, st + 5 + torch.rand(b, generator=g) * 30], -1).reshape(b, 1, 2), "m_duration": torch.full((b,), 100.0),
                "v_duration": torch.full((b,), 9.0), "video_id": ["v"] * b, "music_id": ["m"] * b}
        data = {"frame_feats": torch.zeros(b, 2, 4), "frame_mask": torch.ones(b, 2), "segment_feats": torch.zeros(b, 3, 4), "segment_mask": torch.ones(b, 3)}
        batches.append((data, meta, torch.zeros(b, 1, 2)))
    args = _args(["--mml_localization", "regression", "--max_m_duration", "100", "--num_display", "3", "--epochs", "1"])
    args.rank, args.world_size, args.total_step = 0, 1, 0
    lines = []
    logger = logging.getLogger("deferred-reads-test")
    logger.setLevel(logging.INFO)
    h = logging.Handler()
    h.emit = lambda rec: lines.append(rec.getMessage())
    logger.addHandler(h)
    reads = [0]
    for name in ("__float__", "item", "tolist", "cpu", "numpy"):      # every way a value leaves a tensor for the host
        def counted(self, *a, _orig=getattr(torch.Tensor, name), **kw):
            reads[0] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    model = _Canned(steps, reads)
    loss, metrics = driver.train_one_epoch(1, args, model, batches, None, torch.device("cpu"), None, logger, n_steps, 0)
    monkeypatch.undo()
    # display points follow steps 2, 4 and 6: no value is read between two steps without one in between
    at = model.reads_at
    assert at[0] == at[1] and at[2] == at[3] and at[4] == at[5] and at[2] > at[1]
    # the per-step formula
    meter, ious, want_lines = {"loss": 0.0, "ret": 0.0, "loc": 0.0, "n": 0}, [], []
    for k, (o, (data, meta, _)) in enumerate(zip(steps, batches)):
        ret, loc = o["ret"][0] * args.ret_loss_weight, o["loc"][0] * args.loc_loss_weight
        ious.extend(driver._batch_iou(args, model, {"pred_spans": o["spans"]}, meta, torch.device("cpu")).cpu().tolist())
        b = sizes[k]
        meter["loss"] += float(ret + loc) * b; meter["ret"] += float(ret) * b; meter["loc"] += float(loc) * b; meter["n"] += b
        if (k + 1) % max(1, n_steps // 3) == 0:
            want_lines.append(f"Train [1/1, {k + 1}/{n_steps}] loss {meter['loss'] / meter['n']:.4f} ret {meter['ret'] / meter['n']:.4f} "
                              f"loc {meter['loc'] / meter['n']:.4f} ")
    assert model.k == n_steps and args.total_step == n_steps
    assert loss == meter["loss"] / meter["n"]
    assert metrics == IoU_metrics(ious) and metrics["mIoU"] > 0
    assert len(lines) == len(want_lines) == 3
    for got, want in zip(lines, want_lines):
        assert got.startswith(want), (got, want)
