"""Scalar restatement of the cut rule (include/made_hip.h, "Cuts"): made_frame_hist, made_hist_distance and made_cut_peaks in plain
Python over numpy int64, one step of the rule per line, written apart from mgsv_amd/cuts.py's vectorised `backend="host"`.  Also
the synthetic videos the CPU and GPU tests share: shots with planted cuts, and one shaking shot."""
import numpy as np


def frame_hist_ref(frame):
    """hist int64 [16, 64] of one frame uint8 [H, W, 3]"""
    H, W = frame.shape[:2]
    px = frame.astype(np.int64)
    Y = (77 * px[:, :, 0] + 150 * px[:, :, 1] + 29 * px[:, :, 2] + 128) >> 8
    b = Y >> 2
    r, c = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    cell = 4 * ((4 * r) // H) + (4 * c) // W
    hist = np.zeros((16, 64), np.int64)
    np.add.at(hist, (cell, b), 1)                                  # one pixel at a time
    return hist


def video_hist_ref(frames):
    """int64 [F, 16, 64]"""
    return np.stack([frame_hist_ref(f) for f in frames]) if len(frames) else np.zeros((0, 16, 64), np.int64)


def distance_ref(hist, first_of_video):
    """D int64 [n] of hist [n, 16, 64]"""
    n = len(hist)
    D = np.zeros(n, np.int64)
    for f in range(1, n):
        if not first_of_video[f]:
            D[f] = int(np.abs(hist[f].astype(np.int64) - hist[f - 1].astype(np.int64)).sum())
    return D


def peaks_ref(D, thr, w_max, w_avg, ratio_q8):
    """(frames, strengths) of one video's distances: lists of Python ints, ascending"""
    D = [int(x) for x in D]
    F = len(D)
    frames, strengths = [], []
    for f in range(F):
        x = D[f]
        if not (x >= int(thr) and x > 0):
            continue
        if any(not x > D[g] for g in range(max(f - w_max, 0), f)):
            continue
        if any(not x >= D[g] for g in range(f + 1, min(f + w_max, F - 1) + 1)):
            continue
        window = [g for g in range(max(f - w_avg, 1), min(f + w_avg, F - 1) + 1) if g != f]
        S, n = sum(D[g] for g in window), len(window)
        if n == 0 or 256 * x * n >= int(ratio_q8) * S:
            frames.append(f)
            strengths.append(x)
    return frames, strengths


def video_cuts_ref(frames, thr, w_max, w_avg, ratio_q8):
    """(D, cut frames, strengths) of one video's frames by the three steps"""
    first = np.zeros(len(frames), np.uint8)
    first[:1] = 1
    D = distance_ref(video_hist_ref(frames), first)
    return (D,) + peaks_ref(D, thr, w_max, w_avg, ratio_q8)


# ------------------------------------------------------------------------------------------------ synthetic videos
SHOTS = (40, 25, 60, 13, 50)
PLANTED = [40, 65, 125, 138]             # the first frame of every shot but the first
SIZES = ((48, 64), (90, 160), (37, 53))


def _shot_image(rng, h, w):
    """a random 8 x 8-block image, box-smoothed once, with a per-shot gain in [0.5, 1] and an offset that keeps it in [0, 255]"""
    blocks = rng.uniform(0, 255, ((h + 7) // 8, (w + 7) // 8, 3))
    img = np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1)[:h, :w]
    pad = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge")
    img = sum(pad[i:i + h, j:j + w] for i in range(3) for j in range(3)) / 9.0
    gain = rng.uniform(0.5, 1.0)
    return img * gain + rng.uniform(0.0, 255.0 * (1.0 - gain))


def _view(rng, img, y, x, H, W):
    return np.clip(np.rint(img[y:y + H, x:x + W] + rng.uniform(-2.0, 2.0, (H, W, 3))), 0, 255).astype(np.uint8)


def planted_video(H, W, seed, shots=SHOTS):
    """uint8 [sum(shots), H, W, 3]: every shot its own image seen through an H x W window that pans 1 px every second frame, uniform
    noise in [-2, 2] on every frame"""
    rng = np.random.default_rng(seed)
    out = []
    for n in shots:
        img = _shot_image(rng, H + 8, W + n // 2 + 8)
        for i in range(n):
            out.append(_view(rng, img, 4, i // 2, H, W))
    return np.stack(out)


def shaky_video(H, W, seed, n=120):
    """one shot whose window jumps by up to +-6 px per frame in both directions (a walk kept inside a 32 px margin): no cut, large
    distances throughout"""
    rng = np.random.default_rng(seed)
    img = _shot_image(rng, H + 32, W + 32)
    y = x = 16
    out = []
    for _ in range(n):
        y, x = (int(np.clip(p + rng.integers(-6, 7), 0, 32)) for p in (y, x))
        out.append(_view(rng, img, y, x, H, W))
    return np.stack(out)
