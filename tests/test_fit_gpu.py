"""GPU: made_fit_moments against the numpy float32 restatement of tests/fit_ref.py, bit for bit (int32 views, so NaNs compare too):
random entries of every kind at sizes around the block, planted edges of the snap rule, length fitting with a NULL table, guard
elements around the four outputs, and the refusals."""
import numpy as np
import pytest
import torch

import fit_ref as FR
from mgsv_amd import _lib, ops

pytestmark = pytest.mark.gpu

f32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(got, want):
    for name, a, b in zip(("out_start", "out_end", "shift", "onset"), got, want):
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        bad = np.flatnonzero(a.view(np.int32) != b.view(np.int32))
        assert len(bad) == 0, (name, bad[:5], a[bad[:5]], b[bad[:5]])


def _device(case, tol):
    start, end, track, want, tlen, ostart, otime = case
    out = ops.fit_moments(dev(start), dev(end), dev(track), dev(want), dev(tlen), dev(ostart), dev(otime), tol)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("per_track", [0, 1, 2, 3, 1000])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 1000])
def test_fit_moments_is_the_numpy_restatement(E, per_track):
    case = FR.random_case(E, 5, per_track, seed=31 * E + per_track)
    for tol in (0.0, 0.05, 3.0):
        got = _device(case, tol)
        _same_bits(got, FR.fit_reference(*case, tol=tol))
        _same_bits(got, ops.fit_moments(*case, tol=tol, backend="host"))
    if E == 1000:
        start, end, track, want = case[:4]
        assert (track < 0).any() and np.isnan(start).any() and np.isnan(end).any() and np.isnan(want).any() and (want == 0).any()
        assert (want > case[4][np.maximum(track, 0)]).any() and (start < 0).any() and (end > case[4][np.maximum(track, 0)]).any()
        if per_track == 1000:
            assert int((got[3] >= 0).sum()) > 300


def test_planted_edges():
    tol = f32(0.5)
    at = f32(40.0) + tol
    lists = [[at], [np.nextafter(at, f32(100))], [39.75, 40.25], [39.75, 40.125], [90.25], [89.75], [0.25], []]
    ostart = np.concatenate([[0], np.cumsum([len(o) for o in lists])]).astype(np.int64)
    otime = np.concatenate([np.asarray(o, f32) for o in lists]).astype(f32)
    start = np.array([40, 40, 40, 40, 85, 85, -8, 40], f32)
    end = np.array([50, 50, 50, 50, 105, 105, 4, 50], f32)
    track = np.arange(8, dtype=np.int32)
    want = np.full(8, 10.0, f32)
    tlen = np.full(8, 100.0, f32)
    case = (start, end, track, want, tlen, ostart, otime)
    got = _device(case, float(tol))
    _same_bits(got, FR.fit_brute_force(*case, tol=float(tol)))
    s, e, sh, w = (a.cpu().numpy() for a in got)
    assert w.tolist() == [0, -1, 0, 1, -1, 0, 0, -1]
    assert s.tolist() == [40.5, 40.0, 39.75, 40.125, 90.0, 89.75, 0.25, 40.0] and e[4] == 100.0 and sh[4] == 5.0


def test_length_alone_with_a_null_table_and_guards():
    start, end, track, want, tlen, _, _ = FR.random_case(333, 7, 0, seed=5)
    E, G = 333, 16
    bufs = [torch.full((E + 2 * G,), -7.0).cuda() for _ in range(3)] + [torch.full((E + 2 * G,), -7, dtype=torch.int32).cuda()]
    args = [dev(a) for a in (start, end, track, want, tlen)]
    st = torch.cuda.current_stream().cuda_stream
    rc = _lib.lib().made_fit_moments(*(a.data_ptr() for a in args[:4]), E, args[4].data_ptr(), 7, None, None, 0, 0.0,
                                     *(b[G:].data_ptr() for b in bufs), st)
    assert rc == 0
    torch.cuda.synchronize()
    _same_bits([b[G:G + E] for b in bufs], FR.fit_reference(start, end, track, want, tlen))
    for b in bufs:
        assert (b[:G] == -7).all() and (b[G + E:] == -7).all()
    got = ops.fit_moments(*args)                                   # the wrapper without a table
    torch.cuda.synchronize()
    _same_bits(got, FR.fit_reference(start, end, track, want, tlen))


def test_refusals():
    a = torch.zeros(4).cuda()
    t = torch.zeros(4, dtype=torch.int32).cuda()
    one = torch.ones(1).cuda()
    for tol in (-1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.MadeError, match="tol"):
            ops.fit_moments(a, a, t, a, one, tol=tol)
    l = _lib.lib()
    p = a.data_ptr()
    assert l.made_fit_moments(p, p, t.data_ptr(), p, 4, one.data_ptr(), 1, None, None, 0, 0.5, p, p, p, t.data_ptr(), None) == -1
    assert b"onset table" in l.made_last_error()
    assert l.made_fit_moments(p, p, t.data_ptr(), p, 4, one.data_ptr(), 1, None, None, 0, 0.0, p, p, None, t.data_ptr(), None) == -1
    assert l.made_fit_moments(p, p, t.data_ptr(), p, 1 << 31, one.data_ptr(), 1, None, None, 0, 0.0, p, p, p, t.data_ptr(), None) == -1
    assert l.made_fit_moments(p, p, t.data_ptr(), p, 0, one.data_ptr(), 1, None, None, 0, 0.0, p, p, p, t.data_ptr(), None) == 0
