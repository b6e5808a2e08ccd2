"""CPU: the frame-feature extractor without a GPU -- PIL's bicubic taps and torchvision's crop offsets as mgsv_amd/frames.py computes
them against an independent numpy restatement that itself reproduces PIL, the reference's frame selection rule, the ViT-B/32
state-dict loader, and the argument validation of made_frames_preprocess (rejected before any HIP call)."""
import os

import numpy as np
import pytest
import torch

import frames_ref as R
from mgsv_amd import _lib


def test_numpy_restatement_matches_pil():
    for i, (h, w) in enumerate(R.SIZES):
        img = R.random_frame(h, w, seed=i)
        rh, rw = R.np_resized_size(h, w)
        t, l = R.np_crop_offsets(rh, rw)
        assert np.array_equal(R.np_resize(img, rh, rw)[t:t + 224, l:l + 224], R.pil_crop(img)), (h, w)


def test_sizes_and_crop_offsets():
    from mgsv_amd import frames as F
    for h, w in R.SIZES + [(225, 225), (226, 227), (1081, 1920), (1, 1)]:
        assert F.resized_size(h, w) == R.np_resized_size(h, w)
        rh, rw = F.resized_size(h, w)
        assert F.crop_offsets(rh, rw) == R.np_crop_offsets(rh, rw)
    assert F.crop_offsets(225, 224) == (0, 0) and F.crop_offsets(227, 224) == (2, 0)      # round(0.5) = 0, round(1.5) = 2
    assert F.resized_size(720, 1280) == (224, 398) and F.resized_size(1280, 720) == (398, 224)


def test_coefficient_tables_match_restatement():
    """The block made_frames_preprocess reads (crop folded in) == the restatement's taps at the cropped outputs; an axis already
    at 224 is a single unit tap at the crop position."""
    from mgsv_amd import frames as F
    for h, w in R.SIZES:
        blk, kh, kv = F.frame_tables(h, w)
        rh, rw = F.resized_size(h, w)
        top, left = F.crop_offsets(rh, rw)
        assert blk.dtype == np.int32 and blk.size == 224 * (4 + kh + kv)
        for rows, k, n_in, n_out, start in ((blk[:224 * (2 + kh)].reshape(224, 2 + kh), kh, w, rw, left),
                                            (blk[224 * (2 + kh):].reshape(224, 2 + kv), kv, h, rh, top)):
            if n_in == n_out:
                assert k == 1 and np.array_equal(rows[:, 0], np.arange(start, start + 224)) and (rows[:, 1] == 1).all()
                assert (rows[:, 2] == 1 << 22).all()
                continue
            xmin, cnt, kk = R.np_taps(n_in, n_out)
            sl = slice(start, start + 224)
            assert kk.shape[1] == k
            assert np.array_equal(rows[:, 0], xmin[sl]) and np.array_equal(rows[:, 1], cnt[sl])
            assert np.array_equal(rows[:, 2:], kk[sl])
            assert (rows[:, 0] >= 0).all() and (rows[:, 0] + rows[:, 1] <= n_in).all()


def test_frame_selection_rule(tmp_path):
    from PIL import Image
    from mgsv_amd import frames as F

    def make(n, end=False, mode="RGB"):
        d = tmp_path / f"v{n}_{int(end)}_{mode}"
        d.mkdir()
        names = [f"{i}.jpg" for i in range(n - 1)] + (["end.jpg"] if end else [f"{n - 1}.jpg"])
        for j, nm in enumerate(names):
            arr = R.random_frame(36, 48, seed=j)
            im = Image.fromarray(arr if mode == "RGB" else arr[..., 0])
            im.save(d / nm, quality=95)
        return str(d)

    d = make(10)
    assert [os.path.basename(p) for p in F.frame_paths(d, 0.3, 6.9, 50)] == [f"{i}.jpg" for i in range(7)]
    assert [os.path.basename(p) for p in F.frame_paths(d, 2.0, 30.0, 50)] == [f"{i}.jpg" for i in range(2, 10)]   # clamp to n - 1
    assert len(F.frame_paths(d, 0.0, 30.0, 5)) == 5                                      # clamp to max_v_frames - 1
    with pytest.raises(ValueError):                                                    # window longer than max_v_frames
        F.frame_indices(100, -10.0, 30.0, 20)
    de = make(6, end=True)
    ps = F.frame_paths(de, 0.0, 5.5, 50)
    assert [os.path.basename(p) for p in ps] == ["0.jpg", "1.jpg", "2.jpg", "3.jpg", "4.jpg", "end.jpg"]
    fr = F.load_video_frames(de, 0.0, 5.5, 50)
    assert len(fr) == 6 and fr[0].shape == (36, 48, 3) and fr[0].dtype == np.uint8
    assert np.array_equal(fr[5], np.asarray(Image.open(os.path.join(de, "end.jpg")).convert("RGB")))
    dl = make(3, mode="L")                                                            # L -> RGB: three equal channels
    g = F.load_video_frames(dl, 0.0, 2.0, 50)
    assert g[0].shape == (36, 48, 3) and np.array_equal(g[0][..., 0], g[0][..., 2])
    dm = tmp_path / "cmyk"
    dm.mkdir()
    Image.new("CMYK", (8, 8)).save(dm / "0.jpg")
    with pytest.raises(ValueError):
        F.load_video_frames(str(dm), 0.0, 0.0, 50)
    dmiss = tmp_path / "missing"
    dmiss.mkdir()
    for nm in ("0.jpg", "2.jpg", "3.jpg"):
        Image.new("RGB", (8, 8)).save(dmiss / nm)
    with pytest.raises(RuntimeError):
        F.frame_paths(str(dmiss), 0.0, 2.0, 50)


def _sd():
    from mgsv_amd import synth
    return synth.make_clip_visual_state_dict(seed=3)


def test_state_dict_loader(tmp_path):
    from mgsv_amd import frames as F
    sd = _sd()
    flat = {k[len("visual."):]: v for k, v in sd.items()}
    # an OpenAI-style TorchScript archive: fp16 tensors under visual.*, text-tower keys beside them
    root = torch.nn.Module()
    for k, v in list(sd.items()) + [("positional_embedding", torch.zeros(77, 512)), ("token_embedding.weight", torch.zeros(10, 512))]:
        mod = root
        parts = k.split(".")
        for p in parts[:-1]:
            if not hasattr(mod, p):
                mod.add_module(p, torch.nn.Module())
            mod = getattr(mod, p)
        mod.register_parameter(parts[-1], torch.nn.Parameter(v.half(), requires_grad=False))
    path = str(tmp_path / "ViT-B-32.pt")
    torch.jit.script(root).save(path)
    a = F.load_visual_state_dict(path)
    assert set(a) == set(flat) and all(a[k].dtype == torch.float32 for k in a)
    assert torch.equal(a["conv1.weight"], flat["conv1.weight"].half().float())
    for src in (sd, flat):                                                           # prefixed / unprefixed dicts
        b = F.load_visual_state_dict(src)
        assert all(torch.equal(b[k], flat[k]) for k in flat)
    p2 = str(tmp_path / "plain.pt")
    torch.save(flat, p2)
    assert torch.equal(F.load_visual_state_dict(p2)["proj"], flat["proj"])
    bad = dict(flat)
    bad["proj"] = torch.zeros(768, 768)                                              # ViT-L/14-like projection width
    with pytest.raises(ValueError, match="proj"):
        F.load_visual_state_dict(bad)
    deeper = dict(flat)
    deeper["transformer.resblocks.12.ln_1.weight"] = torch.ones(768)                 # a 13th block: another architecture
    with pytest.raises(ValueError, match="ViT-B/32"):
        F.load_visual_state_dict(deeper)
    short = {k: v for k, v in flat.items() if k != "ln_post.bias"}
    with pytest.raises(ValueError, match="missing"):
        F.load_visual_state_dict(short)


def _lib_built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


FAKE = 4096          # a non-null "device pointer": validation rejects the call before anything reads it


def _pre(l, frames=FAKE, nbytes=1000, desc=FAKE, n=4, coef=FAKE, ncoef=1000, patches=FAKE, dt=0, ld=3072, crop=None):
    return l.made_frames_preprocess(frames, nbytes, desc, n, coef, ncoef, patches, dt, ld, crop, None)


def test_frames_preprocess_rejects_bad_arguments():
    l = _lib_built()
    bad = -1                                                        # MADE_ERR_INVALID_ARG
    assert _pre(l, frames=None) == bad
    assert _pre(l, desc=None) == bad
    assert _pre(l, coef=None) == bad
    assert _pre(l, patches=None) == bad
    assert _pre(l, n=-1) == bad
    assert _pre(l, n=(1 << 20) + 1) == bad                          # too many frames
    assert "n_frames" in l.made_last_error().decode()
    assert _pre(l, nbytes=0) == bad
    assert _pre(l, ncoef=0) == bad
    assert _pre(l, dt=2) == bad
    assert _pre(l, ld=3071) == bad
    assert _pre(l, n=0) == 0                                        # nothing to do: no launch
