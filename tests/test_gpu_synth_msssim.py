"""GPU checks of dvie_synth_msssim through synth.frame_msssim / frame_scores(msssim=) and the
held-out scoring above them, against the float64 CPU restatement of the definition
(tests/msssim_ref.py).

Shapes: 177x183 at 5 scales (levels 177x183, 88x91, 44x45, 22x22, 11x11: odd at three levels;
level 0 has three 64-pixel strips and six 32-row segments, ragged at every level), 90x150 at 4
scales with lead (2, 2) and pred a transposed view of slot-major storage, 37x53 at 2 scales and
at 1 with buffers that start 1 byte into their allocation.

Gates: (1) parts against the truth, 1e-4 absolute per scale -- the gate of the same kind of
mean in test_gpu_synth_score.py; (2) msssim against float64 numpy on the device's own parts, 1e-12
relative; (3) msssim against the truth within the per-scale gate propagated through the product,
want * sum_s w_s * 1e-4 / parts_truth[s], where the truth's smallest scale is at least 0.02 (every
case but 0 against 255, whose last scale is ~1e-5); (4) identical frames within 1e-6 of 1; (5) one
scale within 1e-4 of frame_scores' ssim.

Measured worst deviations (MI355X; DESIGN.md "Multi-scale SSIM" has the table): parts 2.7e-7
(177x183 random, level 3) and 6.2e-6 for 0 against 255; msssim against numpy on the device's parts
2e-16 relative; msssim against the truth 1.4e-7; identical frames exactly 1."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd.synth import (VideoSynthesizer, frame_msssim, frame_scores,
                                                              msssim_weights)
from msssim_ref import msssim_truth
from test_gpu_synth_score import CONTENTS, _frames, _labels, _offset_by_one, _slot_major
from test_gpu_synth_score_video import _clip, _net

pytestmark = pytest.mark.gpu

# name -> (lead, H, W, scales)
CASES = {"177x183k5": ((2,), 177, 183, 5), "90x150k4": ((2, 2), 90, 150, 4), "37x53k2": ((3,), 37, 53, 2),
         "37x53k1": ((3,), 37, 53, 1)}


@functools.lru_cache(maxsize=None)
def _case(name, content):
    """inputs and truth of one (case, content): computed once, shared, never modified"""
    lead, H, W, K = CASES[name]
    pred, gt = _frames(lead, H, W, content, 300 + 10 * list(CASES).index(name) + CONTENTS.index(content))
    truth = [msssim_truth(a, b, K) for a, b in zip(pred.reshape(-1, H, W, 3), gt.reshape(-1, H, W, 3))]
    return pred, gt, np.stack([t[0] for t in truth]), np.array([t[1] for t in truth])


def _to_dev(name, pred, gt, dev):
    if name.startswith("37x53"):
        return _offset_by_one(pred, dev), _offset_by_one(gt, dev)
    if name.startswith("90x150"):  # pred: a slot-major view; gt: plain (B, S) storage
        return _slot_major(pred, dev), torch.from_numpy(gt).to(dev)
    return torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("name", list(CASES))
def test_frame_msssim_against_the_float64_truth(dev, name, content):
    lead, H, W, K = CASES[name]
    pred, gt, want_parts, want = _case(name, content)
    p, g = _to_dev(name, pred, gt, dev)
    ms_t, parts_t = frame_msssim(p, g, K)
    assert ms_t.dtype == torch.float64 and tuple(ms_t.shape) == lead
    assert parts_t.dtype == torch.float64 and tuple(parts_t.shape) == lead + (K,)
    ms, parts = ms_t.cpu().numpy().ravel(), parts_t.cpu().numpy().reshape(-1, K)
    w = np.array(msssim_weights(K), dtype=np.float64)
    d_parts = np.abs(parts - want_parts)
    own = np.prod(np.maximum(parts, 0.0) ** w, axis=1)
    print(f"msssim {name} {content}: max |parts - truth| per scale = "
          f"{' '.join(f'{x:.2e}' for x in d_parts.max(axis=0))}, max |msssim - truth| = {np.abs(ms - want).max():.3e}, "
          f"max rel |msssim - numpy(parts)| = {(np.abs(ms - own) / np.maximum(own, 1e-300)).max():.2e}, "
          f"min truth part = {want_parts.min():.3e}")
    assert (d_parts <= 1e-4).all(), (parts, want_parts)  # gate 1
    assert (np.abs(ms - own) <= 1e-12 * own).all(), (ms, own)  # gate 2
    for f in range(len(ms)):  # gate 3
        if want_parts[f].min() >= 0.02:
            bound = want[f] * float(np.sum(w * 1e-4 / want_parts[f]))
            assert abs(ms[f] - want[f]) <= bound, (f, ms[f], want[f], bound)
    if content != "black_white":
        assert (want_parts.min(axis=1) >= 0.02).all(), want_parts  # (gate 3 was applied to every frame)
    if content == "identical":  # gate 4
        assert (np.abs(1 - ms) <= 1e-6).all(), ms
    if K == 1:  # gate 5
        ssim = frame_scores(p, g).ssim.cpu().numpy().ravel()
        print(f"msssim {name} {content}: max |msssim - frame_scores ssim| = {np.abs(ms - ssim).max():.3e}")
        assert (np.abs(ms - ssim) <= 1e-4).all() and (np.abs(parts[:, 0] - ssim) <= 1e-4).all(), (ms, ssim)


def test_two_calls_give_the_same_bytes(dev):
    pred, gt, _, _ = _case("177x183k5", "random")
    p, g = _to_dev("177x183k5", pred, gt, dev)
    a, b = frame_msssim(p, g, 5), frame_msssim(p, g, 5)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_guard_bytes_around_outputs_and_workspace(dev):
    """the raw entry point on buffers fenced with guard values: both outputs and the workspace
    (exactly dvie_synth_msssim_ws_bytes bytes) are written inside their bounds only, and the
    results are frame_msssim's"""
    name = "37x53k2"
    lead, H, W, K = CASES[name]
    n = lead[0]
    pred, gt, want_parts, _ = _case(name, "noise6")
    p, g = _to_dev(name, pred, gt, dev)
    ref_ms, ref_parts = frame_msssim(p, g, K)
    lib = L.load()
    d = L.SynthMsssimDesc()
    d.pred, d.gt, d.n0, d.n1, d.h, d.w, d.scales = p.data_ptr(), g.data_ptr(), 1, n, H, W, K
    d.pred_s1 = d.gt_s1 = H * W * 3
    G = 4  # guard words on each side
    GUARD = -0x0123456789ABCDEF
    bufs = {k: torch.full((m + 2 * G,), GUARD, dtype=torch.int64, device=dev) for k, m in (("msssim", n), ("parts", n * K))}
    for k, t in bufs.items():
        setattr(d, k, t.data_ptr() + 8 * G)
    nbytes = lib.dvie_synth_msssim_ws_bytes(ctypes.byref(d))
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
    d.ws = ws.data_ptr() + 32
    L.check(lib.dvie_synth_msssim(ctypes.byref(d), L.stream_ptr(dev)), "synth msssim")
    torch.cuda.synchronize()
    for k, t in bufs.items():
        h = t.cpu().numpy()
        assert (h[:G] == GUARD).all() and (h[-G:] == GUARD).all(), k
    assert bufs["msssim"].cpu().numpy()[G:-G].tobytes() == ref_ms.cpu().numpy().tobytes()
    assert bufs["parts"].cpu().numpy()[G:-G].tobytes() == ref_parts.cpu().numpy().tobytes()
    assert (np.abs(ref_parts.cpu().numpy() - want_parts) <= 1e-4).all()
    w = ws.cpu().numpy()
    assert (w[:32] == 0xA5).all() and (w[-32:] == 0xA5).all()


def test_frame_scores_with_msssim_keyword(dev):
    name = "37x53k2"
    lead, H, W, K = CASES[name]
    pred, gt, _, _ = _case(name, "noise6")
    pl, gl = _labels(lead, H, W, 9)
    p, g = _to_dev(name, pred, gt, dev)
    a, b = _offset_by_one(pl, dev), _offset_by_one(gl, dev)
    plain, both = frame_scores(p, g, a, b), frame_scores(p, g, a, b, msssim=2)
    assert plain.msssim is None and plain.vgg is None and both.vgg is None
    assert both.msssim.cpu().numpy().tobytes() == frame_msssim(p, g, 2)[0].cpu().numpy().tobytes()
    for k in ("sse", "ssim", "agree", "valid", "inter", "uni"):
        x, y = getattr(plain, k), getattr(both, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), k


def test_argument_errors(dev):
    f = torch.zeros((2, 175, 200, 3), dtype=torch.uint8, device=dev)
    for K in (0, 6):
        with pytest.raises(ValueError, match="scales"):
            frame_msssim(f, f, K)
    with pytest.raises(ValueError, match="at most 4 scales"):
        frame_msssim(f, f, 5)
    with pytest.raises(ValueError, match="at most 4 scales"):
        frame_scores(f, f, msssim=5)
    with pytest.raises(ValueError):
        frame_msssim(f.float(), f, 2)
    with pytest.raises(ValueError):
        frame_msssim(f, f.float(), 2)
    with pytest.raises(ValueError):
        frame_msssim(f, f[:1], 2)


# ---------------- held-out scoring and the launcher ----------------
H, W, NC = 32, 64, 20


def test_score_interpolation_carries_msssim(dev):
    model = _net("inter", "fp32").to(dev).eval()
    frames, labels = _clip(2, 5, H, W, 61)
    syn = VideoSynthesizer(model, max_batch=2)
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    sc = syn.score_interpolation(f, l, levels=1, msssim=2)
    plain = syn.score_interpolation(f, l, levels=1)
    assert sc.slots == [1, 3] and tuple(sc.msssim.shape) == (2, 2) and sc.msssim.dtype == torch.float64
    assert plain.msssim is None and plain.scores.msssim is None
    for j, t in enumerate(sc.slots):
        want = frame_msssim(sc.frames[:, t], f[:, t], 2)[0]
        assert sc.msssim[:, j].cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), t
    for k in ("sse", "ssim", "agree", "valid", "inter", "uni"):
        assert torch.equal(getattr(sc, k), getattr(plain, k)), k
    v = sc.msssim.cpu().numpy()
    summ, base = sc.summary(), plain.summary()
    assert summ["msssim"] == float(np.mean(v.ravel())) and "msssim" not in base
    pos = np.asarray(sc.positions)
    for p, row in summ["per_position"].items():
        assert row["msssim"] == float(np.mean(v[:, pos == p].ravel())), p
    assert np.array_equal(sc.host(msssim=True)[4], v) and len(sc.host()) == 4
    assert {k: x for k, x in summ.items() if k not in ("msssim", "per_position")} == \
        {k: x for k, x in base.items() if k != "per_position"}
    with pytest.raises(ValueError, match="at most 2 scales"):
        syn.score_interpolation(f, l, levels=1, msssim=3)


def test_score_extrapolation_carries_msssim(dev):
    model = _net("extra", "fp32").to(dev).eval()
    frames, labels = _clip(2, 4, H, W, 63)
    syn = VideoSynthesizer(model, max_batch=2)
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    sc = syn.score_extrapolation(f, l, msssim=2)
    assert tuple(sc.msssim.shape) == (2, 2)
    want = frame_msssim(sc.frames, f[:, 2:], 2)[0]
    assert sc.msssim.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()


def _keys(x):
    if isinstance(x, dict):
        return set(x) | {k for v in x.values() for k in _keys(v)}
    if isinstance(x, list):
        return {k for v in x for k in _keys(v)}
    return set()


def _launch(tmp_path, dev, extra, tag, size=(H, W)):
    from PIL import Image
    from deep_video_interpolation_extrapolation_amd import main as M
    h, w = size
    frames, labels = _clip(1, 3, h, w, 71, ignore=False)
    data = tmp_path / f"data_{tag}"
    for sub in ("rgb", "seg"):
        (data / sub / "aachen_000001").mkdir(parents=True)
    for t in range(3):
        Image.fromarray(frames[0, t]).save(data / "rgb" / "aachen_000001" / f"{t:02d}.png")
        Image.fromarray(labels[0, t]).save(data / "seg" / "aachen_000001" / f"{t:02d}.png")
    model = _net("inter", "fp32", seed=7).to(dev).eval()
    run = tmp_path / f"run_{tag}"
    (run / "checkpoint").mkdir(parents=True)
    torch.save({"session": 0, "epoch": 2, "coarse_model": model.coarse_model.state_dict()},
               run / "checkpoint" / "InterNet_xs2xs_inter_0_1_0.pth")
    M.main(["--split", "test", "--synth_eval", "--syn_type", "inter", "--input_h", str(h), "--input_w", str(w),
            "--precision", "fp32", "--load_dir", str(run), "--checksession", "0", "--checkepoch", "1",
            "--checkpoint", "0", "--cycgen_load_dir", str(data)] + extra + ["INTER", "--load_coarse"])
    return json.loads((data / "synth_eval" / "scores.json").read_text()), model, frames, labels


def test_main_launcher_synth_msssim(dev, tmp_path):
    got, model, frames, labels = _launch(tmp_path, dev, ["--synth_msssim", "2"], "ms")
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    sc = VideoSynthesizer(model, max_batch=1).score_interpolation(f, l, levels=1, msssim=2)
    assert list(got) == ["clips", "summary", "msssim_scales"] and got["msssim_scales"] == 2
    row = got["clips"]["aachen_000001"]
    assert list(row) == ["slots", "psnr", "ssim", "acc", "miou", "msssim"] and row["slots"] == sc.slots == [1]
    for k in ("psnr", "ssim", "acc", "miou", "msssim"):
        assert row[k] == getattr(sc, k)[0].cpu().numpy().tolist(), k
    assert 0.0 < row["msssim"][0] < 1.0
    assert got["summary"]["msssim"] == float(np.mean(row["msssim"]))
    for p, r in got["summary"]["per_position"].items():
        assert r["msssim"] == float(np.mean(row["msssim"])), p
    # without the flag: no such key anywhere
    plain, *_ = _launch(tmp_path, dev, [], "plain")
    assert list(plain) == ["clips", "summary"]
    assert not [k for k in _keys(plain) if str(k).startswith("msssim")]
    assert list(plain["clips"]["aachen_000001"]) == ["slots", "psnr", "ssim", "acc", "miou"]
    for k in ("slots", "psnr", "ssim", "acc", "miou"):
        assert plain["clips"]["aachen_000001"][k] == row[k], k
    # a clip too small for the scales asked for ends the run, named
    with pytest.raises(ValueError, match=r"aachen_000001: .*at most 2 scales"):
        _launch(tmp_path, dev, ["--synth_msssim", "3"], "small")
