"""CPU: MadeTrainer._step_body holds the order of a training iteration for the eager step and every recorder of TrainStepGraph.  It depends
on its trainer only through forward_train, backward, optimizer_step and group_ranges, so a stub that logs those calls shows the order of
events of each caller's policy, and that all of them see one bucket boundary.  No library, no device."""
import pytest

from mgsv_amd.trainer import MadeTrainer, bucket_cut

CUT = 1200
BATCH = ("frames", "segments", "frame_masks", "segment_masks", "spans")
LRS = (1e-3, 2e-3, 3e-3)


class StubTrainer:
    """the three calls of a step append to `events`; backward invokes the hooks it is given at its grad_sync point, as the real one does"""
    group_ranges = ((0, CUT), (CUT, 5000), (5000, 9000))

    def __init__(self):
        self.events = []

    def forward_train(self, *batch, seed, music_ids, v_duration, zero_grad):
        assert batch == BATCH
        self.events.append(("forward", seed, zero_grad))
        return {"out": seed}

    def backward(self, g_ret, g_loc, grad_sync=None, early_opt=None):
        self.events.append(("backward", g_ret, g_loc))
        if grad_sync is not None:
            grad_sync()
        if early_opt is not None:
            early_opt()
        self.events.append(("backward ends",))

    def optimizer_step(self, *lrs, part=None, **kw):
        self.events.append(("optimizer", lrs, part, kw))


def _run(**policy):
    stub = StubTrainer()
    opt_kw = policy.pop("opt_kw", dict(max_grad_norm=0.5))
    out = MadeTrainer._step_body(stub, BATCH, 7, LRS, opt_kw, **policy)
    assert out == {"out": 7}
    return stub.events


def test_bucket_cut_is_the_end_of_the_temporal_group():
    assert bucket_cut(StubTrainer.group_ranges) == CUT


def test_plain_step_runs_forward_backward_optimizer_once_each():
    assert _run(w_ret="wr", w_loc="wl") == [("forward", 7, True), ("backward", "wr", "wl"), ("backward ends",),
                                            ("optimizer", LRS, None, dict(max_grad_norm=0.5))]


def test_data_parallel_step_reduces_the_large_bucket_inside_backward_and_the_temporal_one_behind_it():
    seen = []
    ev = _run(opt_kw=dict(max_grad_norm=0.5, grad_scale=0.25), grad_sync=lambda cut: seen.append(("large bucket from", cut)),
              after_backward=lambda cut: seen.append(("temporal bucket up to", cut)))
    assert seen == [("large bucket from", CUT), ("temporal bucket up to", CUT)]
    assert ev == [("forward", 7, True), ("backward", None, None), ("backward ends",),
                  ("optimizer", LRS, None, dict(max_grad_norm=0.5, grad_scale=0.25))]


def test_hooks_fire_between_the_stages_they_name():
    order = []
    stub = StubTrainer()
    stub.events = order
    MadeTrainer._step_body(stub, BATCH, 7, LRS, {}, grad_sync=lambda cut: order.append(("grad_sync", cut)),
                           after_backward=lambda cut: order.append(("after_backward", cut)))
    assert [e[0] for e in order] == ["forward", "backward", "grad_sync", "backward ends", "after_backward", "optimizer"]


def test_two_part_step_applies_the_early_part_inside_backward_and_the_rest_behind_it():
    ev = _run(early=True)
    assert ev == [("forward", 7, True), ("backward", None, None), ("optimizer", LRS, "early", dict(max_grad_norm=0.5)), ("backward ends",),
                  ("optimizer", LRS, "rest", dict(max_grad_norm=0.5))]


@pytest.mark.parametrize("fill_in_forward", [True, False])
def test_capture_style_step_reads_the_device_state_and_switches_at_both_hooks(fill_in_forward):
    """what TrainStepGraph's recorders pass: zero learning rates and a device_state, hooks that move the capture on; the three-graph
    capture alone leaves the gradient fill to backward (fill_in_forward=False)"""
    state, seen = object(), []
    opt_kw = dict(max_grad_norm=1.0, grad_scale=0.5, device_state=state)
    stub = StubTrainer()
    MadeTrainer._step_body(stub, BATCH, 0, (0.0, 0.0, 0.0), opt_kw, fill_in_forward=fill_in_forward, grad_sync=seen.append, after_backward=seen.append)
    assert seen == [CUT, CUT]
    assert stub.events == [("forward", 0, fill_in_forward), ("backward", None, None), ("backward ends",),
                           ("optimizer", (0.0, 0.0, 0.0), None, opt_kw)]
    assert stub.events[-1][3]["device_state"] is state


def test_data_parallel_hooks_reduce_two_buckets_then_wait_for_both():
    """MadeTrainer._dp_hooks with a recording stand-in for torch.distributed: issued at once (eager) and through a `defer` that, like
    tape.callback, runs the collective now and keeps it for replays"""
    log, kept = [], []

    class Work:
        def __init__(self, name):
            self.name = name

        def wait(self):
            log.append(("wait", self.name))

    class Dist:
        @staticmethod
        def all_reduce(part, async_op):
            assert async_op
            log.append(("all_reduce", part))
            return Work(part)

    stub = StubTrainer()
    stub.flat_grad = "abcdefgh"
    stub.group_ranges = ((0, 3), (3, 6), (6, 8))
    hooks = MadeTrainer._dp_hooks(stub, Dist, defer=lambda fn: (kept.append(fn), fn()))
    MadeTrainer._step_body(stub, BATCH, 7, LRS, {}, **hooks)
    want = [("all_reduce", "defgh"), ("all_reduce", "abc"), ("wait", "defgh"), ("wait", "abc")]
    assert log == want and len(kept) == 3
    del log[:]
    for fn in kept:                                          # a replay: the same collectives again, and nothing left over from the first run
        fn()
    assert log == want
