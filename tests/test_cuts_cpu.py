"""CPU: cut detection without a GPU -- `detect_cuts(backend="host")` against tests/cuts_ref.py's scalar restatement bit for bit, the
invariants of the three steps, planted cuts and a shaking shot, hand-built distance sequences, max_cuts, the refusals, the way into
`Fit(cuts=)`, `frames.load_frame_sequence` and tools/detect_cuts.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cuts_ref as CR
from mgsv_amd import cuts as CU, frames as FR, ops
from mgsv_amd.cuts import Cuts, detect_cuts
from mgsv_amd.grounding import Fit

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPS = 32.0                               # the defaults then give w_max = 8, w_avg = 32
SEEDS = 20


def _rows(table, name="frame"):
    return [getattr(table, name)[table.start[v]:table.start[v + 1]] for v in range(len(table))]


@pytest.fixture(scope="module")
def planted():
    """per size: (videos, the host backend's table, the reference's (D, frames, strengths) per video); computed once, read-only"""
    out = {}
    for H, W in CR.SIZES:
        videos = [CR.planted_video(H, W, seed) for seed in range(SEEDS)]
        table = detect_cuts(videos, FPS, backend="host")
        assert table.params["w_max"][0] == 8 and table.params["w_avg"][0] == 32 and table.params["ratio_q8"] == 768
        thr = int(np.ceil(0.25 * 2 * H * W))
        out[(H, W)] = (videos, table, [CR.video_cuts_ref(v, thr, 8, 32, 768) for v in videos])
    return out


def test_host_backend_is_the_scalar_restatement(planted):
    for (H, W), (videos, table, ref) in planted.items():
        for v, (D, frames, strengths) in enumerate(ref):
            s, e = table.start[v], table.start[v + 1]
            assert table.frame[s:e].tolist() == frames
            assert np.array_equal(table.strength[s:e], (np.asarray(strengths, np.float64) / (2 * H * W)).astype(f32))
            assert np.array_equal(table.time[s:e], np.asarray(frames, f32) / f32(FPS))
        # the steps one by one, on a few videos
        for vid, (D, _, _) in list(zip(videos, ref))[:3]:
            hist = CU.frame_hist_host(vid)
            assert np.array_equal(hist, CR.video_hist_ref(vid))
            first = np.zeros(len(vid), np.uint8)
            first[0] = 1
            assert np.array_equal(CU.hist_distance_host(hist, first), D)


def test_invariants_of_the_signature_and_the_distance(planted):
    for (H, W), (videos, _, ref) in planted.items():
        vid = videos[0]
        hist = CU.frame_hist_host(vid)
        assert (hist >= 0).all() and (hist.reshape(len(vid), -1).sum(axis=1) == H * W).all()
        D = ref[0][0]
        assert D[0] == 0 and (D >= 0).all() and (D <= 2 * H * W).all()
    still = np.repeat(videos[0][:1], 5, axis=0)                     # identical frames
    first = np.array([1, 0, 0, 0, 0], np.uint8)
    assert not CU.hist_distance_host(CU.frame_hist_host(still), first).any()
    assert not CR.distance_ref(CR.video_hist_ref(still), first).any()
    # the first frame of a video in the middle of a batch
    two = np.concatenate([videos[0][:3], videos[1][:3]])
    flags = np.array([1, 0, 0, 1, 0, 0], np.uint8)
    for D in (CU.hist_distance_host(CU.frame_hist_host(two), flags), CR.distance_ref(CR.video_hist_ref(two), flags)):
        assert D[0] == 0 and D[3] == 0 and D[1] > 0 and D[4] > 0
    # disjoint bins: exactly 2 P
    a = np.zeros((2, 6, 10, 3), np.uint8)
    a[1] = 255
    assert CU.hist_distance_host(CU.frame_hist_host(a), np.array([1, 0], np.uint8)).tolist() == [0, 120]
    # cells of a 3 x 3 frame: rows and columns 0, 1, 2 fall into cells 0, 1, 2 of 4 -- seven of the sixteen cells stay empty
    h = CU.frame_hist_host(np.zeros((1, 3, 3, 3), np.uint8))[0]
    assert np.array_equal(h, CR.frame_hist_ref(np.zeros((3, 3, 3), np.uint8)))
    assert sorted(np.flatnonzero(h.sum(axis=1)).tolist()) == [0, 1, 2, 4, 5, 6, 8, 9, 10]


def test_planted_cuts_are_found_and_nothing_else(planted):
    """The margins come from the generator, measured on the reference: over the 60 videos the smallest planted-cut strength was 0.40
    and the largest strength of any other frame 0.147 (threshold 0.25).  Asserted with room on either side of the threshold -- a
    planted cut changes at least 0.30 of the picture, no other frame more than 0.20 -- so that a change of generator cannot make
    the test vacuous."""
    smallest, largest = 1.0, 0.0
    for (H, W), (videos, table, ref) in planted.items():
        for v, (D, frames, _) in enumerate(ref):
            s = D / (2.0 * H * W)
            smallest = min(smallest, s[CR.PLANTED].min())
            other = s.copy()
            other[CR.PLANTED] = 0
            largest = max(largest, other.max())
            assert frames == CR.PLANTED, (H, W, v, frames)
            assert table.frame[table.start[v]:table.start[v + 1]].tolist() == CR.PLANTED
    print(f"smallest planted-cut strength {smallest:.3f}, largest other strength {largest:.3f}")
    assert smallest >= 0.30 and largest <= 0.20


def test_a_shaking_shot_has_no_cut_and_rule_3_is_what_says_so():
    videos = [CR.shaky_video(48, 64, seed) for seed in range(SEEDS)]
    assert len(detect_cuts(videos, FPS, backend="host").time) == 0
    loose = detect_cuts(videos, FPS, backend="host", ratio=0.0)       # the same threshold, rule 3 switched off
    print(f"cuts in {SEEDS} shaking shots with ratio = 0: {len(loose.time)}")
    assert len(loose.time) > 0
    thr = int(np.ceil(0.25 * 2 * 48 * 64))
    for v, vid in enumerate(videos[:4]):
        for q8, table in ((768, None), (0, loose)):
            _, frames, _ = CR.video_cuts_ref(vid, thr, 8, 32, q8)
            assert frames == ([] if table is None else _rows(table)[v].tolist())


def _both(D, thr, w_max, w_avg, q8):
    ref = CR.peaks_ref(D, thr, w_max, w_avg, q8)
    got = CU.cut_peaks_host(np.asarray(D), thr, w_max, w_avg, q8)
    assert got[0].tolist() == ref[0] and got[1].tolist() == ref[1]
    return ref[0]


def test_hand_built_distance_sequences():
    assert _both([0, 5, 5, 5, 0], 1, 2, 2, 0) == [1]                # equal neighbours: the earlier wins
    assert _both([0, 5, 0, 5, 0], 1, 2, 2, 0) == [1]                # ... also at the window's far end
    assert _both([0, 5, 0, 0, 5], 1, 2, 2, 0) == [1, 4]             # w_max + 1 apart: both
    assert _both([0, 9], 1, 1, 1, 65535) == [1]                     # n = 0: frame 0 is left out of the window, the test passes
    assert _both([7, 9], 1, 1, 1, 65535) == [1]                     # ... whatever D[0] holds
    assert _both([0, 9, 1], 1, 1, 1, 256 * 9) == [1]                # 256 * 9 * 1 >= 2304 * 1
    assert _both([0, 9, 1], 1, 1, 1, 256 * 9 + 1) == []
    assert _both([0, 0, 0, 0, 0, 0, 8], 1, 3, 4, 768) == [6]        # windows clipped at the end
    assert _both([0, 8, 0, 0, 0, 0, 0], 1, 3, 4, 768) == [1]        # ... and at the beginning
    assert _both([0, 8, 3, 3, 3, 3, 3], 1, 3, 4, 768) == []         # 256 * 8 * 4 < 768 * 12
    assert _both([0, 8, 3, 3, 3, 3, 3], 1, 3, 4, 682) == [1]        # 8192 >= 682 * 12 = 8184
    assert _both([0, 8, 3], 9, 1, 1, 0) == []                       # below the threshold
    assert _both([0, 0, 0], 0, 1, 1, 0) == []                       # D > 0 even with a zero threshold
    assert _both([9, 1, 1], 1, 1, 1, 0) == [0]                      # the kernel's rule on any D; detect_cuts' D[0] is 0
    for F in (0, 1, 2):
        assert _both([0, 4][:F], 1, 8, 32, 768) == ([1] if F == 2 else [])
    rng = np.random.default_rng(0)
    for case in range(40):
        F = int(rng.integers(0, 400))
        D = rng.integers(0, 50, F) * rng.integers(0, 2, F) if case % 2 else np.full(F, 7)
        _both(D, int(rng.integers(0, 30)), int(rng.choice([1, 8, 64])), int(rng.choice([1, 32, 128])), int(rng.choice([0, 768, 65535])))


def test_videos_of_zero_one_and_two_frames():
    rng = np.random.default_rng(1)
    a, b = np.zeros((1, 5, 7, 3), np.uint8), np.full((1, 5, 7, 3), 255, np.uint8)
    videos = [np.zeros((0, 5, 7, 3), np.uint8), a, np.concatenate([a, b]), rng.integers(0, 256, (0, 2, 2, 3)).astype(np.uint8)]
    table = detect_cuts(videos, [FPS, 10.0, 4.0, 1.0], backend="host")
    assert table.start.tolist() == [0, 0, 0, 1, 1] and table.frame.tolist() == [1] and table.strength.tolist() == [1.0]
    assert table.time.tolist() == [0.25] and table.of(2).tolist() == [0.25] and len(table) == 4
    assert table.params["w_max"] == [8, 3, 1, 1] and table.params["w_avg"] == [32, 10, 4, 1]
    assert len(detect_cuts([], FPS, backend="host")) == 0


def test_max_cuts_keeps_the_strongest_the_earlier_of_equal_ones_ascending():
    frame, strength = np.array([3, 9, 20, 31, 44], np.int32), np.array([50, 70, 50, 90, 50], np.int64)
    assert [a.tolist() for a in CU._strongest(frame, strength, 3)] == [[3, 9, 31], [50, 70, 90]]
    assert [a.tolist() for a in CU._strongest(frame, strength, 4)] == [[3, 9, 20, 31], [50, 70, 50, 90]]
    assert CU._strongest(frame, strength, 5)[0] is frame and CU._strongest(frame, strength, 1)[0].tolist() == [31]
    # through detect_cuts: flashes of different size, one frame in three
    vid = np.zeros((30, 8, 8, 3), np.uint8)
    for i, f in enumerate(range(3, 30, 6)):                         # the frame turns white over (i % 3 + 4) rows, and back
        vid[f, :i % 3 + 4] = 255
    every = detect_cuts([vid], 4.0, backend="host", ratio=0.0)
    assert every.frame.tolist() == [3, 9, 15, 21, 27] and every.strength.tolist() == [0.5, 0.625, 0.75, 0.5, 0.625]
    kept = detect_cuts([vid], 4.0, backend="host", ratio=0.0, max_cuts=3)
    assert kept.frame.tolist() == [9, 15, 27] and kept.strength.tolist() == [0.625, 0.75, 0.625]
    assert kept.time.tolist() == [2.25, 3.75, 6.75]
    assert detect_cuts([vid], 4.0, backend="host", ratio=0.0, max_cuts=4).frame.tolist() == [3, 9, 15, 27]


def test_refusals_come_before_anything_is_computed():
    ok = np.zeros((3, 4, 4, 3), np.uint8)
    bad_videos = [np.zeros((3, 4, 4, 3), np.float32), np.zeros((3, 4, 4), np.uint8), np.zeros((3, 4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.uint8),
                  np.zeros((3, 0, 4, 3), np.uint8), torch.zeros(3, 4, 4, 3), [[1, 2, 3]],
                  np.lib.stride_tricks.as_strided(np.zeros(3, np.uint8), (1, 4097, 4096, 3), (0, 0, 0, 1))]     # P = 2^24 + 4096
    for backend in ("host", "device"):                              # ("device" must refuse before it touches a GPU)
        for v in bad_videos:
            with pytest.raises(ValueError):
                detect_cuts([ok, v], FPS, backend=backend)
        for fps in (0.0, -1.0, float("nan"), float("inf"), [FPS], [FPS, FPS, FPS], [FPS, 0.0], [[FPS, FPS]]):
            with pytest.raises(ValueError, match="fps"):
                detect_cuts([ok, ok], fps, backend=backend)
        for kw in (dict(threshold=0.0), dict(threshold=1.5), dict(threshold=-0.1), dict(threshold=float("nan")), dict(min_shot=0.0),
                   dict(min_shot=-1.0), dict(context=0.0), dict(context=float("nan")), dict(ratio=-0.5), dict(ratio=255.5),
                   dict(ratio=float("nan")), dict(max_cuts=0), dict(max_cuts=-3)):
            with pytest.raises(ValueError, match=next(iter(kw))):
                detect_cuts([ok], FPS, backend=backend, **kw)
    with pytest.raises(ValueError, match="backend"):
        detect_cuts([ok], FPS, backend="eager")
    detect_cuts([ok], FPS, backend="host", threshold=1.0, ratio=255.0, max_cuts=1)      # the ends of the ranges are allowed
    with pytest.raises(ValueError):
        Cuts(np.array([0, 2]), np.array([1.0], f32), np.array([1]), np.array([0.5]))


def test_fit_takes_the_table(planted):
    videos, table, _ = planted[(37, 53)]
    fit = Fit("video", snap=0.5, cuts=table)
    start, time = fit._cut_csr
    assert np.array_equal(start, table.start) and np.array_equal(time, table.time) and time.dtype == np.float32
    as_lists = Fit("video", snap=0.5, cuts=[table.of(v) for v in range(len(table))])
    assert np.array_equal(as_lists._cut_csr[0], start) and np.array_equal(as_lists._cut_csr[1], time)
    assert (time > 0).all() and all((np.diff(table.of(v)) > 0).all() for v in range(len(table)))
    frames = np.arange(1, 65, dtype=np.int32)
    many = Cuts(np.array([0, 64]), frames.astype(f32) / f32(FPS), frames, np.full(64, 0.5, f32))
    with pytest.raises(ValueError, match="64 cuts"):
        Fit("video", snap=0.5, cuts=many)
    with pytest.raises(ValueError, match="64 cuts"):
        Fit("video", snap=0.5, cuts=[many.time])
    assert ops.SYNC_MAX_CUTS == 63 and detect_cuts.__defaults__[5] == 63


# ---------------------------------------------------------------------------------------------- frames on disk, the tool
@pytest.fixture()
def frame_dirs(tmp_path):
    """two videos as directories of small JPEGs: "a" with the files 0, 1, 2, ..., 11 (a cut at frame 6), "b" with 0 .. 3"""
    from PIL import Image
    rng = np.random.default_rng(0)
    texture = np.repeat(np.repeat(rng.integers(0, 56, (6, 8, 1)), 4, axis=0), 4, axis=1)          # 4 x 4 blocks over 14 luma bins
    for name, n, cut in (("a", 12, 6), ("b", 4, None)):
        os.makedirs(tmp_path / name)
        for i in range(n):
            level = 40 if cut is None or i < cut else 190
            img = np.broadcast_to(texture + level + i, (24, 32, 3)).astype(np.uint8)              # a slow brightening: the order shows
            Image.fromarray(img).save(str(tmp_path / name / f"{i}.jpg"), quality=95)
    return tmp_path


def test_load_frame_sequence_reads_in_numeric_order(frame_dirs):
    d = str(frame_dirs / "a")
    seq = FR.load_frame_sequence(d)
    assert seq.shape == (12, 24, 32, 3) and seq.dtype == np.uint8
    for i in (0, 1, 2, 10, 11):                                     # 10.jpg comes after 2.jpg, not after 1.jpg
        assert np.array_equal(seq[i], FR.decode_frame(os.path.join(d, f"{i}.jpg")))
    means = seq.reshape(12, -1).mean(axis=1)
    assert (np.diff(means[:6]) > 0).all() and (np.diff(means[6:]) > 0).all()
    part = FR.load_frame_sequence(d, first=2, last=10)
    assert np.array_equal(part, seq[2:11])
    assert FR.load_frame_sequence(d, first=12).shape[0] == 0
    with pytest.raises(RuntimeError, match="12.jpg"):
        FR.load_frame_sequence(d, last=12)
    from PIL import Image
    Image.fromarray(np.zeros((24, 30, 3), np.uint8)).save(os.path.join(d, "12.jpg"))
    with pytest.raises(ValueError, match="12.jpg"):
        FR.load_frame_sequence(d)
    assert FR.load_frame_sequence(d, last=11).shape[0] == 12


def test_the_tool_writes_the_table(frame_dirs, tmp_path):
    out = str(tmp_path / "cuts.json")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "detect_cuts.py"), "--frames_root", str(frame_dirs), "--fps", "4",
                          "--out", out, "--backend", "host"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "2 videos, 1 cuts, 15.00 cuts per minute" in run.stdout
    got = json.load(open(out))
    table = detect_cuts([FR.load_frame_sequence(str(frame_dirs / n)) for n in ("a", "b")], 4.0, backend="host")
    assert table.frame.tolist() == [6]
    assert got == {"a": {"fps": 4.0, "cuts": [1.5], "strength": [float(table.strength[0])]}, "b": {"fps": 4.0, "cuts": [], "strength": []}}
    only = str(tmp_path / "only.json")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "detect_cuts.py"), "--frames_root", str(frame_dirs), "--fps", "4",
                          "--out", only, "--backend", "host", "--ids", "b"], capture_output=True, text=True)
    assert run.returncode == 0 and list(json.load(open(only))) == ["b"]
