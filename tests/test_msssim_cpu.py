"""CPU checks (no launch) of the multi-scale SSIM: the float64 truth helper (tests/msssim_ref.py)
against the oracle's SSIM and against repeated average pooling, the weights and the size rule of
synth, the host-side summary, the --synth_msssim option, and the exports, descriptor size and
argument validation of dvie_synth_msssim."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import synth
from deep_video_interpolation_extrapolation_amd.options import Options
from msssim_ref import WEIGHTS, level, msssim_truth
from oracle.losses import ssim_value


def _pair(H, W, seed):
    rng = np.random.RandomState(seed)
    gt = rng.randint(0, 256, (H, W, 3))
    return np.clip(gt + rng.randint(-20, 21, gt.shape), 0, 255).astype(np.uint8), gt.astype(np.uint8)


# ---------------- the truth helper ----------------
@pytest.mark.parametrize("H,W", [(37, 53), (11, 11), (5, 7)])
def test_truth_at_one_scale_is_the_oracle_ssim(H, W):
    pred, gt = _pair(H, W, 1)
    if min(H, W) < 11:  # (the size rule of the multi-scale form; the oracle has none)
        with pytest.raises(AssertionError):
            msssim_truth(pred, gt, 1)
        return
    parts, ms = msssim_truth(pred, gt, 1)
    t = lambda x: torch.from_numpy(x).permute(2, 0, 1)[None].double() / 255  # noqa: E731
    want = float(ssim_value(t(pred), t(gt)))
    assert parts.shape == (1,) and abs(parts[0] - want) <= 1e-12 and abs(ms - want) <= 1e-12


def test_truth_pyramid_is_repeated_avg_pool_bit_for_bit():
    pred, _ = _pair(45, 51, 2)  # odd at levels 0, 1 (22x25) and 2 (11x12)
    # pooling the byte values is exact in float64 (integer sums times a power of two), so the
    # pooled image over 255 and the block sum over 255 * 4**s are one rounding of one number
    y = torch.from_numpy(pred).permute(2, 0, 1)[None].double()
    for s in range(4):
        got = level(pred, s)
        assert got.dtype == torch.float64 and tuple(got.shape) == (1, 3, 45 >> s, 51 >> s)
        assert torch.equal(got, y / 255.0), s
        y = F.avg_pool2d(y, 2)


def test_truth_identical_frames_give_exactly_one():
    _, gt = _pair(44, 47, 3)
    for K in (1, 2, 3):
        parts, ms = msssim_truth(gt.copy(), gt, K)
        assert (parts == 1.0).all() and ms == 1.0, K


def test_truth_clamps_a_negative_scale_to_zero():
    rng = np.random.RandomState(4)
    a = rng.randint(0, 256, (24, 24, 3)).astype(np.uint8)
    parts, ms = msssim_truth(a, 255 - a, 2)  # an inverted frame: negative structure at the fine scale
    assert parts[0] < 0 and ms == 0.0


# ---------------- synth: weights, size rule ----------------
def test_weights_sum_to_one_and_are_the_published_vector():
    assert synth.MSSSIM_WEIGHTS == WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    for K in range(1, 6):
        w = synth.msssim_weights(K)
        assert len(w) == K and abs(sum(w) - 1.0) <= 2.0 ** -52
        assert all(abs(a * sum(WEIGHTS[:K]) - b) <= 2.0 ** -53 for a, b in zip(w, WEIGHTS))
    assert synth.msssim_weights(1) == (1.0,)
    # K = 5: the published vector (which sums to 1.0001) over its sum
    assert synth.msssim_weights(5) == tuple(x / sum(WEIGHTS) for x in WEIGHTS)
    for K in (0, 6):
        with pytest.raises(ValueError):
            synth.msssim_weights(K)


def test_max_scales_and_the_size_rule():
    assert [synth.msssim_max_scales(n, 4096) for n in (176, 175, 11, 10)] == [5, 4, 1, 0]
    assert [synth.msssim_max_scales(4096, n) for n in (176, 175, 11, 10)] == [5, 4, 1, 0]
    assert synth.msssim_max_scales(88, 87) == 3 and synth.msssim_max_scales(1024, 2048) == 5
    synth.msssim_check(176, 300, 5)
    with pytest.raises(ValueError, match="at most 4 scales"):
        synth.msssim_check(175, 200, 5)
    with pytest.raises(ValueError, match="at most 0 scales"):
        synth.msssim_check(10, 200, 1)
    for K in (0, 6, 2.0, True, None):
        with pytest.raises(ValueError):
            synth.msssim_check(256, 256, K)


def test_frame_msssim_refuses_cpu_tensors():
    f = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(L.DvieError):
        synth.frame_msssim(f, f, 1)


# ---------------- summary, FrameScores, option ----------------
def test_summarize_with_and_without_msssim():
    rng = np.random.RandomState(5)
    pos = np.array([1, 2, 3] * 4)
    psnr, ssim, acc, miou, vgg, ms = rng.rand(6, 12)
    base = synth.summarize(pos, psnr, ssim, acc, miou)
    assert "msssim" not in base and all("msssim" not in r for r in base["per_position"].values())
    assert base == synth.summarize(pos, psnr, ssim, acc, miou, msssim=None)
    s = synth.summarize(pos, psnr, ssim, acc, miou, msssim=ms)
    assert s["msssim"] == float(np.mean(ms)) and list(s)[:6] == ["psnr", "ssim", "acc", "miou", "msssim", "frames"]
    for p, row in s["per_position"].items():
        assert row["msssim"] == float(np.mean(ms[pos == p]))
        assert {k: v for k, v in row.items() if k != "msssim"} == base["per_position"][p]
    assert {k: v for k, v in s.items() if k not in ("msssim", "per_position")} == \
        {k: v for k, v in base.items() if k != "per_position"}
    both = synth.summarize(pos, psnr, ssim, acc, miou, vgg=vgg, msssim=ms)
    assert list(both)[:7] == ["psnr", "ssim", "acc", "miou", "vgg", "msssim", "frames"]
    assert both["vgg"] == float(np.mean(vgg)) and both["msssim"] == s["msssim"]


def test_frame_scores_fields_carry_msssim():
    assert "msssim" in synth.FrameScores.FIELDS and len(synth.FrameScores.FIELDS) == 8
    t = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    fs = synth.FrameScores(4, 4, t.long(), t)
    assert fs.msssim is None and fs.vgg is None and fs.map(lambda x: x + 1).msssim is None
    fs = synth.FrameScores(4, 4, t.long(), t, msssim=t)
    assert torch.equal(fs.map(lambda x: x[:, 1]).msssim, t[:, 1])
    sc = synth.SynthScores([1, 2, 3], [1, 2, 3], fs, None, None)
    assert sc.msssim is fs.msssim and sc.vgg is None
    with pytest.raises(ValueError, match="msssim"):
        synth.SynthScores([1], [1], synth.FrameScores(4, 4, t.long(), t), None, None).host(msssim=True)


def test_option_synth_msssim():
    base = ["--split", "test", "--synth_eval"]
    assert Options().parse(base + ["INTER"]).synth_msssim == 0
    assert Options().parse(["EXTRA"]).synth_msssim == 0
    assert Options().parse(base + ["--synth_msssim", "3", "INTER"]).synth_msssim == 3
    a = Options().parse(base + ["--synth_msssim", "5", "--synth_vgg", "EXTRA"])
    assert a.synth_msssim == 5 and a.synth_vgg is True


# ---------------- C ABI ----------------
def _desc(**kw):
    """a valid descriptor of 2x3 pairs of 177x183 at 5 scales (the pointers are never followed)"""
    d = L.SynthMsssimDesc()
    base = dict(pred=64, gt=64, msssim=64, parts=64, ws=64, n0=2, n1=3, h=177, w=183, scales=5)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_symbols_and_descriptor_size():
    lib = L.load()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dvie_[a-z0-9_]+)", out))
    for name in ("dvie_synth_msssim", "dvie_synth_msssim_ws_bytes"):
        assert name in exported and name in L.EXPORTS and hasattr(lib, name), name
    assert L._ABI_MORE[111] is L.SynthMsssimDesc
    assert lib.dvie_abi_sizeof(111) == ctypes.sizeof(L.SynthMsssimDesc) == 96


@pytest.mark.parametrize("kw,word", [
    (dict(pred=None), b"null"), (dict(gt=None), b"null"),
    (dict(scales=0), b"scales"), (dict(scales=6), b"scales"),
    (dict(h=175, w=200), b"at most 4 scales"), (dict(h=10, scales=1), b"at most 0 scales"),
    (dict(h=0), b"must be in"), (dict(w=(1 << 19) + 1), b"must be in"),
    (dict(msssim=None), b"msssim"), (dict(parts=None), b"parts"), (dict(ws=None), b"workspace"),
    (dict(n0=0), b"frames"), (dict(n0=256, n1=256), b"frames"),
    (dict(ws=68), b"aligned"), (dict(msssim=68), b"aligned"), (dict(parts=68), b"aligned"),
])
def test_argument_validation_without_gpu(kw, word):
    lib = L.load()
    assert lib.dvie_synth_msssim(ctypes.byref(_desc(**kw)), None) == L.DVIE_EINVAL, kw
    assert word in lib.dvie_last_error(), (kw, lib.dvie_last_error())


def test_workspace_query():
    """8 bytes per level-pass block (64-pixel strips x 32-row segments of every level) and pair,
    then levels 1 .. K-1 of both frames of every pair as uint16, each level padded to 8 bytes"""
    lib = L.load()
    q = lambda **kw: lib.dvie_synth_msssim_ws_bytes(ctypes.byref(_desc(**kw)))  # noqa: E731

    def want(N, H, W, K):
        blocks = sum(-(-(W >> s) // 64) * -(-(H >> s) // 32) for s in range(K))
        pyr = sum(-(-(2 * N * (H >> s) * (W >> s) * 3 * 2) // 8) * 8 for s in range(1, K))
        return 8 * N * blocks + pyr

    assert q() == want(6, 177, 183, 5) == 8 * 6 * (18 + 6 + 2 + 1 + 1) + want(6, 177, 183, 5) - 8 * 6 * 28
    assert q(scales=1) == 8 * 6 * 18
    assert q(h=90, w=150, n0=2, n1=2, scales=4) == want(4, 90, 150, 4)
    assert q(h=37, w=53, n0=1, n1=3, scales=2) == want(3, 37, 53, 2)
    assert q(h=11, w=11, n0=1, n1=1, scales=1) == 8
    assert q(scales=0) == 0 and q(scales=6) == 0 and q(h=175) == 0 and q(n0=0) == 0 and q(w=0) == 0
