"""CPU checks (no launch) of held-out scoring: the exports and the descriptor size of
dvie_synth_score, its argument validation, the workspace query, the held-out slot lists, the
host-side summary and the --synth_eval option."""
import ctypes

import numpy as np
import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import synth
from deep_video_interpolation_extrapolation_amd.options import Options


def _desc(**kw):
    """a valid descriptor of 2x3 frames of 37x53 with label maps (the pointers are never followed)"""
    d = L.SynthScoreDesc()
    base = dict(pred=64, gt=64, pred_label=64, gt_label=64, sse=64, ssim=64, agree=64, valid=64, inter=64, uni=64, ws=64,
                n0=2, n1=3, h=37, w=53, n_classes=20)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_score_symbols_and_descriptor_size():
    lib = L.load()
    for name in ("dvie_synth_score", "dvie_synth_score_ws_bytes"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert L._ABI[107] is L.SynthScoreDesc
    assert lib.dvie_abi_sizeof(107) == ctypes.sizeof(L.SynthScoreDesc)


@pytest.mark.parametrize("kw,word", [
    (dict(pred=None), b"null"), (dict(gt=None), b"null"),
    (dict(pred_label=None), b"together"), (dict(gt_label=None), b"together"),
    (dict(n_classes=33), b"n_classes"), (dict(n_classes=0), b"n_classes"),
    (dict(h=0), b"at least 1"), (dict(w=0), b"at least 1"), (dict(h=-4), b"at least 1"),
    (dict(ws=None), b"workspace"),
    (dict(sse=None), b"sse"), (dict(ssim=None), b"ssim"), (dict(uni=None), b"uni"),
    (dict(n0=0), b"frames"), (dict(n0=256, n1=256), b"frames"),
    (dict(ws=68), b"aligned"), (dict(ssim=68), b"aligned"),
])
def test_score_argument_validation_without_gpu(kw, word):
    lib = L.load()
    assert lib.dvie_synth_score(ctypes.byref(_desc(**kw)), None) == L.DVIE_EINVAL, kw
    assert word in lib.dvie_last_error(), (kw, lib.dvie_last_error())


def test_score_workspace_query():
    """16 bytes per block (float64 SSIM partial, int64 squared error) plus, with label maps,
    2 + 2 * n_classes uint32 counts; blocks = frames x 64-pixel strips x 32-row segments"""
    lib = L.load()
    q = lambda **kw: lib.dvie_synth_score_ws_bytes(ctypes.byref(_desc(**kw)))  # noqa: E731
    blocks = 6 * 1 * 2
    assert q() == blocks * (16 + 4 * 42)
    assert q(pred_label=None, gt_label=None) == blocks * 16
    assert q(h=70, w=150, n0=1, n1=4, n_classes=3) == 4 * 3 * 3 * (16 + 4 * 8)
    assert q(h=1, w=1, n0=1, n1=1, pred_label=None, gt_label=None) == 16
    assert q(h=0) == 0 and q(w=0) == 0 and q(n_classes=33) == 0 and q(n0=0) == 0


@pytest.mark.parametrize("T,levels,want", [
    (3, 1, [1]), (5, 1, [1, 3]), (5, 2, [1, 2, 3]), (9, 2, [1, 2, 3, 5, 6, 7]), (9, 3, [1, 2, 3, 4, 5, 6, 7]),
    (17, 3, [t for t in range(17) if t % 8]),
])
def test_heldout_slots(T, levels, want):
    got = synth.heldout_slots(T, levels)
    assert got == want
    # the complement of the kept frames, and what midpoint_schedule fills for the kept frames
    kept = list(range(0, T, 1 << levels))
    assert sorted(got + kept) == list(range(T))
    filled = sorted(o for lvl in synth.midpoint_schedule(len(kept), levels) for _, _, o in lvl)
    assert filled == got


@pytest.mark.parametrize("T,levels", [(4, 2), (4, 1), (2, 1), (5, 3), (1, 1), (5, 0), (5, -1)])
def test_heldout_slots_refuses(T, levels):
    with pytest.raises(ValueError):
        synth.heldout_slots(T, levels)


def test_summarize_means_per_position_and_overall():
    rng = np.random.RandomState(3)
    pos = np.array([1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3])
    psnr, ssim, acc, miou = rng.rand(4, 12) * np.array([[40.0], [1.0], [1.0], [1.0]])
    psnr[4] = np.inf
    s = synth.summarize(pos, psnr, ssim, acc, miou)
    assert s["frames"] == 12 and s["psnr"] == float("inf") and isinstance(s["ssim"], float)
    assert s["ssim"] == float(np.mean(ssim)) and s["acc"] == float(np.mean(acc)) and s["miou"] == float(np.mean(miou))
    assert sorted(s["per_position"]) == [1, 2, 3]
    for p in (1, 2, 3):
        row = s["per_position"][p]
        assert row["frames"] == 4 and row["ssim"] == float(np.mean(ssim[pos == p]))
        assert row["psnr"] == float(np.mean(psnr[pos == p]))
    assert s["per_position"][2]["psnr"] == float("inf") and np.isfinite(s["per_position"][1]["psnr"])


def test_frame_scores_refuses_cpu_tensors_and_bad_arguments():
    f = torch.zeros((2, 5, 7, 3), dtype=torch.uint8)
    with pytest.raises(L.DvieError):
        synth.frame_scores(f, f)


def test_options_parse_with_and_without_synth_eval():
    a = Options().parse(["--split", "test", "INTER"])
    assert a.synth_eval is False and a.synth_levels == 1
    a = Options().parse(["--split", "test", "--synth_eval", "--synth_levels", "2", "INTER", "--load_coarse"])
    assert a.synth_eval is True and a.synth_levels == 2 and a.runner == "INTER"
    a = Options().parse(["--synth_eval", "EXTRA", "--num_pred_step", "3"])
    assert a.synth_eval is True and a.num_pred_step == 3
