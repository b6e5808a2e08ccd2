"""CPU: the window tables (mgsv_amd/windows.py) against literal loops, the descriptor builder against music.segment_table of each
window's crop and a counted number of unique segments, the numpy restatement of made_merge_moments (tests/windows_ref.py) against
hand-worked cases, and the new entry points' symbols and argument validation (rejected before any HIP call)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import windows_ref as WR
from mgsv_amd import _lib, music, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("made_gather_rows", "made_group_topw", "made_merge_moments")


@pytest.mark.parametrize("d", [0, 1, 239.99, 240, 240.01, 359, 360, 361, 1000])
def test_window_table_against_a_literal_loop(d):
    window, hop = 240, 120
    n16 = int(round(d * 16000))
    dd = n16 / 16000
    want_off, want_dur = [0.0], [min(window, dd)]
    if dd > window:                                  # windows every hop seconds until one reaches the track's end
        j = 1
        while (j - 1) * hop + window < dd:
            want_off.append(j * hop)
            want_dur.append(min(window, dd - j * hop))
            j += 1
        assert len(want_off) == 1 + math.ceil((dd - window) / hop)
    off, dur = windows.window_table(n16, window, hop, 2.5)
    assert off.tolist() == want_off and dur.tolist() == want_dur
    assert (dur > 0).all() or d == 0
    assert off[-1] + window >= dd                    # the windows cover the track


def test_window_table_counts():
    n = lambda d: len(windows.window_table(int(d * 16000))[0])
    assert [n(d) for d in (0, 1, 240, 240.01, 359, 360, 361, 1000)] == [1, 1, 1, 2, 2, 2, 3, 8]


@pytest.mark.parametrize("hop", [0, -120, 240.5, 119, 1.0])
def test_window_table_refuses_a_bad_hop(hop):
    with pytest.raises(ValueError):
        windows.window_table(16000 * 300, 240, hop, 2.5)


@pytest.mark.parametrize("window,hop", [(240, 120), (20, 10), (20, 20), (30, 7.5)])
@pytest.mark.parametrize("sec", [0.0, 9.0, 47.0, 263.7731, 600.0])
def test_descriptors_are_the_segment_table_of_each_crop(window, hop, sec):
    n16 = int(sec * 16000)
    off, dur = windows.window_table(n16, window, hop, 2.5)
    desc = windows.window_descriptors(n16, window, hop, 2.5, 4.0)
    assert len(desc) == len(off)
    pcm = np.arange(n16)                              # stands for pcm16: the crop is a slice of it
    for j, (first, count, mask) in enumerate(desc):
        a = int(16000 * off[j])
        crop = pcm[a:int(16000 * (off[j] + window))]
        f, c, m, mdur = music.segment_table(len(crop), 2.5, 4.0, 0, window)
        assert np.array_equal(first - a, f) and np.array_equal(count, c) and np.array_equal(mask, m)
        assert abs(mdur - dur[j]) < 1e-9
        assert (first + count <= a + int(16000 * window)).all()       # no segment reads past its window's end


def test_unique_descriptors_of_a_600_s_track():
    window, hop, stride, filt = 240, 120, 2.5, 4.0
    n16 = 600 * 16000
    win, masks, uniq, index = windows.library_descriptors([n16], window, hop, stride, filt)
    # from the definition: 4 windows (0, 120, 240, 360 s) of 96 segments, every centre inside the track; a segment is its samples
    keys, total = set(), 0
    for j in range(4):
        for s in range(96):
            c = s * stride
            start, end = max(0.0, c - filt / 2), min(float(window), c + filt / 2)
            a, b = int(16000 * start), int(16000 * end)
            keys.add((j * hop * 16000 + a, b - a))
            total += 1
    # 240 distinct centres (0 .. 597.5 s) + the first segment of windows 1 .. 3, clipped at the window's start
    assert len(keys) == 243 and total == 384
    assert len(uniq) == win.n_encoded == len(keys) and len(uniq) < int(masks.sum()) == total
    assert {(int(f), int(c)) for _, f, c in uniq} == keys
    assert win.track.tolist() == [0] * 4 and win.offset.tolist() == [0, 120, 240, 360] and win.duration.tolist() == [240] * 4
    # the index names, for every (window, segment), the row holding exactly its descriptor
    desc = windows.window_descriptors(n16, window, hop, stride, filt)
    for j, (first, count, mask) in enumerate(desc):
        for s in range(96):
            assert tuple(uniq[index[j * 96 + s]]) == (0, first[s], count[s])


def test_library_descriptors_of_several_tracks():
    n16 = [47 * 16000, 9 * 16000, int(31.3 * 16000)]
    win, masks, uniq, index = windows.library_descriptors(n16, 20, 10, 2.5, 4.0)
    assert win.track.tolist() == [0, 0, 0, 0, 1, 2, 2, 2] and win.n_tracks == 3
    assert (index >= 0).sum() == int(masks.sum()) and index.max() == len(uniq) - 1
    assert np.array_equal((index >= 0).reshape(masks.shape), masks > 0)
    assert (np.diff(uniq[:, 0]) >= 0).all()                       # track-major
    # a short track: one window, the plain segment table
    f, c, m, _ = music.segment_table(n16[1], 2.5, 4.0, 0, 20)
    rows = uniq[index[4 * 8:5 * 8][m > 0]]
    assert np.array_equal(rows[:, 1], f[m > 0]) and np.array_equal(rows[:, 2], c[m > 0]) and (rows[:, 0] == 1).all()


def test_group_csr():
    g = np.array([2, 0, 2, 5, -1, 0, 2], np.int32)
    start, cols = windows.group_csr(g, 4)
    assert start.tolist() == [0, 2, 2, 5, 5] and cols.tolist() == [1, 5, 0, 2, 6]


# ---------------------------------------------------------------------------------------------- the merge restatement, by hand
def _merge(cands, cols, scores, offset, duration=None, n=2, thr=0.5, mx=240.0, use_prob=True):
    cand = np.asarray(cands, np.float32)[None]                    # [1, w, Q, 3]
    return WR.merge_reference(cand, np.asarray([cols], np.int32), np.asarray([scores], np.float32), np.asarray(offset, np.float32),
                              None if duration is None else np.asarray(duration, np.float32), mx, thr, n, use_prob)


def test_merge_identical_spans_from_two_windows_give_one_moment():
    # window 0 (offset 0) sees [150, 170]; window 1 (offset 120) sees the same passage as [30, 50]
    st, en, cf, wi = _merge([[[150, 170, 0.9]], [[30, 50, 0.8]]], [0, 1], [0.7, 0.6], [0, 120])
    assert st[0].tolist()[:1] == [150] and en[0].tolist()[:1] == [170] and wi[0].tolist() == [0, -1]
    assert np.isnan(st[0, 1]) and np.isnan(en[0, 1]) and np.isnan(cf[0, 1]) and cf[0, 0] == np.float32(0.9)
    # the better window wins whatever its probability
    st, en, cf, wi = _merge([[[150, 170, 0.1]], [[30, 50, 0.8]]], [0, 1], [0.5, 0.6], [0, 120])
    assert wi[0].tolist() == [1, -1] and st[0, 0] == 150 and cf[0, 0] == np.float32(0.8)


def test_merge_disjoint_spans_give_both_in_similarity_order():
    st, en, cf, wi = _merge([[[10, 20, 0.2]], [[100, 110, 0.9]]], [3, 4], [0.7, 0.6], [0, 0, 0, 0, 120])
    assert st[0].tolist() == [10, 220] and en[0].tolist() == [20, 230] and wi[0].tolist() == [3, 4]
    # equal similarities: probability decides; equal probabilities: the lower column, then the lower query
    st, en, cf, wi = _merge([[[10, 20, 0.2]], [[100, 110, 0.9]]], [3, 4], [0.7, 0.7], [0, 0, 0, 0, 120])
    assert wi[0].tolist() == [4, 3]
    st, en, cf, wi = _merge([[[10, 20, 0.5], [30, 40, 0.5]], [[100, 110, 0.5], [0, 1, 0.1]]], [4, 3], [0.7, 0.7], [0, 0, 0, 0, 120], n=4)
    assert wi[0].tolist() == [3, 4, 4, 3] and st[0].tolist() == [100, 130, 150, 0]


def test_merge_iou_threshold_is_strict_and_clamps_apply():
    # IoU of [0, 10] and [5, 15] is 5 / 15; of [0, 10] and [0, 20] exactly 0.5: not > 0.5, so kept
    st, en, cf, wi = _merge([[[0, 10, 0.9], [0, 20, 0.8], [1, 10, 0.7]]], [0], [0.5], [0], n=3)
    assert st[0].tolist()[:2] == [0, 0] and en[0].tolist()[:2] == [10, 20] and np.isnan(st[0, 2])      # [1, 10] falls to [0, 10]
    # clamped to [0, min(max_m_duration, duration)] on the window's axis, then shifted
    st, en, cf, wi = _merge([[[-5, 300, 0.9]], [[200, 260, 0.8]]], [0, 1], [0.9, 0.8], [0, 120], duration=[240, 100], mx=240, n=2)
    assert st[0].tolist() == [0, 220] and en[0].tolist() == [240, 220]


def test_merge_zero_length_span_neither_suppresses_nor_is_suppressed():
    st, en, cf, wi = _merge([[[50, 50, 0.9], [40, 60, 0.8], [50, 50, 0.7]]], [0], [0.5], [0], n=3, thr=0.0)
    assert st[0].tolist() == [50, 40, 50] and en[0].tolist() == [50, 60, 50]


def test_merge_more_moments_than_kept_and_missing_windows():
    st, en, cf, wi = _merge([[[10, 20, 0.9]], [[0, 0, 0.99]]], [2, -1], [0.5, -np.inf], [0, 0, 120], n=3)
    assert st[0, 0] == 130 and en[0, 0] == 140 and wi[0].tolist() == [2, -1, -1]
    assert np.isnan(st[0, 1:]).all() and np.isnan(en[0, 1:]).all() and np.isnan(cf[0, 1:]).all()
    st, en, cf, wi = _merge([[[10, 20, 0.9]]], [-1], [-np.inf], [0], n=1)
    assert np.isnan(st[0, 0]) and wi[0, 0] == -1
    # the regression head: no probability key, confidence NaN
    st, en, cf, wi = _merge([[[10, 20, np.nan]], [[30, 40, np.nan]]], [0, 1], [0.5, 0.6], [0, 0], n=2, use_prob=False)
    assert st[0].tolist() == [30, 10] and np.isnan(cf).all()


def test_group_topw_reference_by_hand():
    sims = np.array([[0.5, np.nan, 0.5, -0.0, 0.0, 0.9]], np.float32)
    gid = np.array([0, 0, 0, 1, 1, 2])
    idx, sc = WR.group_topw_reference(sims, np.array([[0, 3, 5, -1]]), gid, 3)
    assert idx[0].tolist() == [[0, 2, 1], [3, 4, -1], [5, -1, -1], [-1, -1, -1]]
    assert np.isnan(sc[0, 0, 2]) and np.isneginf(sc[0, 1, 2]) and np.isneginf(sc[0, 3]).all()


# ---------------------------------------------------------------------------------------------- symbols and validation
def test_new_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "made_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert "windows.hip" in open(os.path.join(ROOT, "mgsv_amd", "csrc", "Makefile")).read()
    assert _lib.lib().made_abi_version() == 9


def test_argument_validation_without_gpu():
    l = _lib.lib()
    one = C.c_void_p(16)                                          # never dereferenced: every call below is refused first
    assert l.made_gather_rows(one, 4, one, 4, 6, one, _lib.F32, None) != 0          # 24-byte rows
    assert b"16-byte" in l.made_last_error()
    assert l.made_gather_rows(one, 4, one, 4, 8, one, 7, None) != 0
    assert l.made_gather_rows(one, 4, None, 4, 8, one, _lib.F32, None) != 0
    for w in (0, 17):
        assert l.made_group_topw(one, 8, one, one, one, one, 8, 2, 8, 3, 2, w, one, one, None) != 0
        assert b"w must lie in [1, 16]" in l.made_last_error()
    assert l.made_group_topw(one, 4, one, one, one, one, 8, 2, 8, 3, 2, 2, one, one, None) != 0     # ld < Nm
    st = l.made_merge_moments(one, one, one, one, None, 4, 8, 16, 17, 1, 240.0, 0.5, 1, one, one, one, one, None)
    assert st != 0 and b"at most 256 candidates" in l.made_last_error()
    assert l.made_merge_moments(one, one, one, one, None, 4, 8, 2, 10, 1, 240.0, -0.1, 1, one, one, one, one, None) != 0
    assert l.made_merge_moments(one, one, one, one, None, 4, 8, 2, 10, 1, 240.0, 0.5, 0, one, one, one, one, None) != 0


def test_merge_moments_has_no_fma_contraction():
    """made_merge_moments is restated in numpy float32 one rounding per operation: csrc/Makefile compiles windows.hip with
    -ffp-contract=off, and the kernel's ISA holds FMAs only inside its one IEEE division (as tests/test_isa_guards_cpu.py checks
    for matcher.hip), the two offset additions, the union's addition and its four subtractions."""
    import subprocess
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    mk = open(os.path.join(ROOT, "mgsv_amd", "csrc", "Makefile")).read()
    assert re.search(r"build/windows\.o:\s*CXXFLAGS\s*\+=\s*-ffp-contract=off", mk)
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-ffp-contract=off", "-S",
                          "--cuda-device-only", "-w", "-o", "-", os.path.join(ROOT, "mgsv_amd", "csrc", "windows.hip")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ins, inside = [], False
    for ln in out.stdout.splitlines():
        if re.match(r"^_Z\w*merge_moments_kernel\w*:", ln):
            inside = True
        elif inside and ln.strip().startswith("s_endpgm"):
            break
        elif inside:
            ins.append(ln.strip())
    assert ins, "merge_moments_kernel not found"
    count = lambda pat: sum(1 for i in ins if re.match(pat, i))
    assert count(r"v_div_fixup_f32") == 1
    assert count(r"v_(fma|fmac|mad)_f32") <= 7                   # the division's expansion
    assert count(r"v_add_f32") == 3 and count(r"v_sub_f32") == 4
