"""CPU checks of scene-cut detection: the numpy restatement (tests/scene_ref.py) at its extremes,
the integer limits at their boundaries, the fill order, the options, the C ABI and its argument
checks, and the margins of the inputs the GPU tests (tests/test_gpu_scene.py) decide on."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import synth
from deep_video_interpolation_extrapolation_amd.options import Options
import scene_ref as R
import yuv_ref as Y


# ---------------- the reference ----------------
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (17, 33)])
def test_reference_extremes(H, W):
    black, white = np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8)
    assert R.luma(white).max() == 255 and R.luma(black).max() == 0  # the weights sum to 256
    sad, hdiff = R.stats(np.stack([black, white, white])[None])
    assert sad.tolist() == [[255 * H * W, 0]] and hdiff.tolist() == [[2 * H * W, 0]]
    rng = np.random.RandomState(H)
    f = rng.randint(0, 256, (2, 3, H, W, 3)).astype(np.uint8)
    sad, hdiff = R.stats(f)
    assert (sad >= 0).all() and (sad <= 255 * H * W).all() and (hdiff >= 0).all() and (hdiff <= 2 * H * W).all()
    assert (hdiff % 2 == 0).all()  # two histograms of one total


def test_limits_are_ceilings_and_the_comparison_is_inclusive():
    assert synth.scene_limits(16, 32, 40, 0.3) == R.limits(16, 32, 40, 0.3) == (20480, 308)
    assert synth.scene_limits(3, 5, 0.1, 0.01) == (2, 1)  # ceil(1.5), ceil(0.3)
    assert synth.scene_limits(1080, 1920, 30, 0.25) == (62208000, 1036800)
    assert synth.scene_limits(4, 4, 0, 0) == (0, 0) and synth.scene_limits(4, 4, 255, 1) == (255 * 16, 32)
    for bad in ((-1, 0.5), (256, 0.5), (30, -0.1), (30, 1.01), (float("nan"), 0.5)):
        with pytest.raises(ValueError):
            synth.scene_limits(4, 4, *bad)
    # a pair that sits exactly on both limits is a cut; one more on either limit and it is not
    H, W = 4, 8
    a = np.zeros((H, W, 3), np.uint8)
    b = a.copy()
    b[0, :4] = 255  # 4 pixels change by 255 and leave bin 0 for bin 31
    f = np.stack([a, b])[None]
    sad, hdiff = (int(v[0, 0]) for v in R.stats(f))
    assert (sad, hdiff) == (4 * 255, 8)
    n = H * W
    assert R.limits(H, W, sad / n, hdiff / (2 * n)) == (sad, hdiff)
    assert R.cuts(f, sad / n, hdiff / (2 * n)).tolist() == [[True]]
    assert R.cuts(f, (sad + 1) / n, hdiff / (2 * n)).tolist() == [[False]]
    assert R.cuts(f, sad / n, (hdiff + 1) / (2 * n)).tolist() == [[False]]
    assert R.limits(H, W, (sad + 1) / n, (hdiff + 1) / (2 * n)) == (sad + 1, hdiff + 1)


def test_cut_sources():
    assert [synth.cut_sources(k) for k in range(4)] == [[], [0], [0, 0, 1], [0, 0, 0, 0, 1, 1, 1]]
    assert all(synth.cut_sources(k) == R.sources(k) for k in range(6))
    with pytest.raises(ValueError):
        synth.cut_sources(-1)


def test_reference_fill_rule():
    slots = np.arange(2 * 9 * 3, dtype=np.uint8).reshape(2, 9, 3)
    got = R.fill(slots, np.array([[True, False], [False, True]]), 2)
    assert np.array_equal(got[0, :, 0] // 3, [0, 0, 0, 4, 4, 5, 6, 7, 8])
    assert np.array_equal(got[1, :, 0] // 3 - 9, [0, 1, 2, 3, 4, 4, 4, 8, 8])


# ---------------- the inputs of the GPU tests ----------------
def _margins(frames, want, what):
    """every pair at least a factor 2 away from both thresholds, on its side"""
    H, W = frames.shape[2:4]
    sad, hdiff = R.stats(frames)
    sad_min, hist_min = R.limits(H, W, R.MAD, R.HIST)
    print(what, "mad", (sad / (H * W)).round(1).tolist(), "hist", (hdiff / (2.0 * H * W)).round(3).tolist())
    assert np.array_equal(R.cuts(frames, R.MAD, R.HIST), want), what
    assert (sad[want] >= 2 * sad_min).all() and (hdiff[want] >= 2 * hist_min).all(), what
    assert (2 * sad[~want] <= sad_min).all() and (2 * hdiff[~want] <= hist_min).all(), what


def test_the_shared_inputs_lie_a_factor_two_from_both_thresholds():
    for H, W in ((16, 32), (15, 30)):
        f, l = R.api_clips(H, W)
        assert f.shape == (2, 4, H, W, 3) and l.shape == (2, 4, H, W) and l.max() < 20
        _margins(f, np.array([[False, True, False], [False] * 3]), f"api {H}x{W}")
    f, _ = R.api_clips(16, 32, T=5, cut_at=3)
    _margins(f, np.array([[False, False, True, False], [False] * 4]), "stream")
    f, _ = R.command_clip()
    want = np.array([[False, False, True, False]])
    _margins(f, want, "command png")
    # the Y4M clip: what the command sees is the conversion of the packed frames
    seen = Y.yuv2rgb_int(Y.rgb2yuv_int(f[0], "C420"), 16, 32, "C420")[None]
    _margins(seen, want, "command y4m")
    # thresholds nothing reaches: 0 against 255 alone does
    assert not R.cuts(R.api_clips()[0], 255, 1).any()


# ---------------- options ----------------
def test_options_synth_scd(capsys):
    a = Options().parse(["INTER"])
    assert a.synth_scd is False and a.synth_scd_mad == 30.0 and a.synth_scd_hist == 0.25
    a = Options().parse(["--synth_scd", "--synth_scd_mad", "40", "--synth_scd_hist", "0.3", "INTER"])
    assert a.synth_scd is True and a.synth_scd_mad == 40.0 and a.synth_scd_hist == 0.3
    a = Options().parse(["--synth_scd_mad", "0", "--synth_scd_hist", "1", "EXTRA"])
    assert a.synth_scd is False and a.synth_scd_mad == 0.0 and a.synth_scd_hist == 1.0
    assert Options().parse(["--synth_scd_mad", "255", "INTER"]).synth_scd_mad == 255.0
    for flag, bad in (("--synth_scd_mad", "-1"), ("--synth_scd_mad", "255.5"), ("--synth_scd_hist", "-0.1"),
                      ("--synth_scd_hist", "1.5"), ("--synth_scd_hist", "x")):
        with pytest.raises(SystemExit):
            Options().parse([flag, bad, "INTER"])
        assert flag in capsys.readouterr().err
    s = synth.SceneCuts()
    assert (s.mad, s.hist) == (30.0, 0.25)
    with pytest.raises(ValueError):
        synth.SceneCuts(mad=256)
    with pytest.raises(ValueError):
        synth.SceneCuts(hist=-0.5)


# ---------------- C ABI ----------------
def test_symbols_and_descriptor_sizes():
    lib = L.load()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dvie_[a-z0-9_]+)", out))
    for name in ("dvie_synth_scene", "dvie_synth_scene_ws_bytes", "dvie_synth_cutfill"):
        assert name in exported and name in L.EXPORTS and hasattr(lib, name), name
    assert L._ABI_MORE[113] is L.SynthSceneDesc and L._ABI_MORE[114] is L.SynthCutFillDesc
    assert lib.dvie_abi_sizeof(113) == ctypes.sizeof(L.SynthSceneDesc) == 88
    assert lib.dvie_abi_sizeof(114) == ctypes.sizeof(L.SynthCutFillDesc) == 56


def _scene_desc(**kw):
    """a valid descriptor of 2 clips of 3 frames of 17x33 (the pointers are never followed)"""
    d = L.SynthSceneDesc()
    base = dict(frames=64, sad=64, hdiff=64, cut=64, ws=64, s0=3 * 17 * 33 * 3, s1=17 * 33 * 3, sad_min=1, hist_min=1,
                n0=2, n1=3, h=17, w=33)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def _fill_desc(**kw):
    d = L.SynthCutFillDesc()
    base = dict(slots=64, cut=64, s0=5 * 100, s1=100, nbytes=100, n0=2, n1=3, levels=1)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,word", [
    (dict(frames=None), b"null"), (dict(sad=None), b"null"), (dict(hdiff=None), b"null"), (dict(ws=None), b"workspace"),
    (dict(n1=1), b"a pair needs two"), (dict(n1=0), b"a pair needs two"), (dict(n0=0), b"clips"),
    (dict(h=0), b"must be in"), (dict(w=0), b"must be in"), (dict(w=(1 << 16) + 1), b"must be in"),
    (dict(sad_min=-1), b"negative"), (dict(hist_min=-1), b"negative"), (dict(ws=68), b"aligned"),
])
def test_scene_argument_validation_without_gpu(kw, word):
    lib = L.load()
    assert lib.dvie_synth_scene(ctypes.byref(_scene_desc(**kw)), None) == L.DVIE_EINVAL, kw
    assert word in lib.dvie_last_error(), (kw, lib.dvie_last_error())


@pytest.mark.parametrize("kw,word", [
    (dict(slots=None), b"null"), (dict(cut=None), b"null"), (dict(nbytes=0), b"nbytes"), (dict(n0=0), b"clips"),
    (dict(n1=1), b"at least 2"), (dict(levels=-1), b"levels"), (dict(levels=9), b"levels"), (dict(s1=99), b"overlap"),
    (dict(n1=65537, levels=1), b"too many"),
])
def test_cutfill_argument_validation_without_gpu(kw, word):
    lib = L.load()
    assert lib.dvie_synth_cutfill(ctypes.byref(_fill_desc(**kw)), None) == L.DVIE_EINVAL, kw
    assert word in lib.dvie_last_error(), (kw, lib.dvie_last_error())


def test_null_descriptors_and_workspace_size():
    lib = L.load()
    assert lib.dvie_synth_scene(None, None) == L.DVIE_EINVAL and b"null" in lib.dvie_last_error()
    assert lib.dvie_synth_cutfill(None, None) == L.DVIE_EINVAL and b"null" in lib.dvie_last_error()
    assert lib.dvie_synth_scene_ws_bytes(None) == 0
    assert lib.dvie_synth_scene_ws_bytes(ctypes.byref(_scene_desc(n1=1))) == 0
    # 17x33 = 561 pixels: one block per clip; 2 x 3 histograms of 32 counts and 2 x 2 SADs, 4 bytes each
    assert lib.dvie_synth_scene_ws_bytes(ctypes.byref(_scene_desc())) == 4 * (6 * 32 + 4)
    # 1080p, 17 frames: ceil(2073600 / 2048) = 1013 blocks
    assert lib.dvie_synth_scene_ws_bytes(ctypes.byref(_scene_desc(n0=1, n1=17, h=1080, w=1920))) == \
        4 * 1013 * (17 * 32 + 16)
    assert lib.dvie_synth_cutfill(ctypes.byref(_fill_desc(levels=0)), None) == L.DVIE_OK  # nothing to fill, no launch


def test_python_entry_points_refuse_cpu_tensors_and_bad_shapes():
    f = torch.zeros((1, 2, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(L.DvieError):
        synth.scene_stats(f)
    with pytest.raises(L.DvieError):
        synth.scene_cuts(f, 30, 0.25)
    with pytest.raises(L.DvieError):
        synth.cut_fill(torch.zeros((1, 3, 8), dtype=torch.uint8), torch.zeros((1, 1), dtype=torch.bool), 1)
