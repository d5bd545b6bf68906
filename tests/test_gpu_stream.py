"""GPU checks of streaming and Y4M: dvie_synth_yuv2rgb / dvie_synth_rgb2yuv against the numpy
restatement of the integer formulas (tests/yuv_ref.py), byte for byte; interpolate_stream against
the per-window and the whole-clip interpolate; the device memory of a streamed clip; and the
`--split test --synth_window` command over a Y4M clip and a PNG clip, with a reader failure."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from deep_video_interpolation_extrapolation_amd import nets, synth
from deep_video_interpolation_extrapolation_amd.synth import VideoSynthesizer, window_plan
from deep_video_interpolation_extrapolation_amd.video_io import Y4MReader, Y4MWriter, frame_bytes
import yuv_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]
SIZES = [(1, 1), (2, 2), (3, 5), (16, 32), (17, 33), (6, 260)]


# ---------------- the kernels ----------------
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("cs", ["C420jpeg", "C444"])
def test_kernels_equal_the_integer_reference(dev, cs, H, W):
    """N = 3 frames of random bytes: an odd-sized packed frame starts at every alignment"""
    N, fb = 3, frame_bytes(W, H, cs)
    rng = np.random.RandomState(1000 * H + W)
    packed = rng.randint(0, 256, (N, fb)).astype(np.uint8)
    rgb = rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    d_packed, d_rgb = torch.from_numpy(packed).to(dev), torch.from_numpy(rgb).to(dev)
    for matrix, full in COMBOS:
        got = synth.yuv_to_rgb(d_packed, H, W, cs, matrix, full)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (N, H, W, 3)
        assert np.array_equal(got.cpu().numpy(), R.yuv2rgb_int(packed, H, W, cs, matrix, full)), (matrix, full)
        got = synth.rgb_to_yuv(d_rgb, cs, matrix, full)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (N, fb)
        assert np.array_equal(got.cpu().numpy(), R.rgb2yuv_int(rgb, cs, matrix, full)), (matrix, full)
    # `out=` of yuv_to_rgb, and the defaults (bt601, limited)
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
    assert synth.yuv_to_rgb(d_packed, H, W, cs, out=out) is out
    assert np.array_equal(out.cpu().numpy(), R.yuv2rgb_int(packed, H, W, cs))


@pytest.mark.parametrize("H,W", [(16, 32), (17, 33), (3, 5)])
@pytest.mark.parametrize("cs", ["C420", "C444"])
def test_rgb_to_yuv_reads_slot_major_views_and_writes_at_an_odd_offset(dev, cs, H, W):
    """frames: the transposed (B, S) view of slot-major (S, B) storage, as interpolate returns it,
    and a strided selection of its slots; out: a slice of a larger buffer at an odd byte offset"""
    S, B, fb = 4, 3, frame_bytes(W, H, cs)
    rng = np.random.RandomState(7 * H + W)
    store = rng.randint(0, 256, (S, B, H, W, 3)).astype(np.uint8)
    d_store = torch.from_numpy(store).to(dev)
    view = d_store.transpose(0, 1)
    assert not view.is_contiguous()
    want = R.rgb2yuv_int(store.transpose(1, 0, 2, 3, 4).reshape(B * S, H, W, 3), cs, "bt709", False)
    big = torch.full((B * S * fb + 9,), 0xA5, dtype=torch.uint8, device=dev)
    out = big[3:3 + B * S * fb].view(B * S, fb)
    assert synth.rgb_to_yuv(view, cs, "bt709", False, out=out) is out
    host = big.cpu().numpy()
    assert np.array_equal(host[3:3 + B * S * fb].reshape(B * S, fb), want)
    assert (host[:3] == 0xA5).all() and (host[3 + B * S * fb:] == 0xA5).all()  # nothing outside the slice
    assert np.array_equal(synth.rgb_to_yuv(view, cs, "bt709", False).cpu().numpy(), want)
    # every other slot of one clip, into every other row of a packed buffer (the command's use)
    rows = torch.zeros((S, fb), dtype=torch.uint8, device=dev)
    synth.rgb_to_yuv(view[1, 1::2], cs, "bt709", False, out=rows[1::2])
    got = rows.cpu().numpy()
    assert np.array_equal(got[1::2], want.reshape(B, S, fb)[1, 1::2]) and (got[0::2] == 0).all()


def test_conversion_argument_checks(dev):
    packed = torch.zeros((2, frame_bytes(32, 16, "C420")), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="Cmono"):
        synth.yuv_to_rgb(packed[:, :512], 16, 32, "Cmono")
    with pytest.raises(ValueError, match="C422"):
        synth.yuv_to_rgb(packed, 16, 32, "C422")
    with pytest.raises(ValueError):
        synth.yuv_to_rgb(packed[:, :-1], 16, 32, "C420")
    with pytest.raises(ValueError):
        synth.rgb_to_yuv(torch.zeros((2, 16, 32, 3), dtype=torch.uint8, device=dev), "C420", "bt601", False, out=packed[:1])
    with pytest.raises(ValueError):
        synth.rgb_to_yuv(torch.zeros((2, 16, 32, 3), dtype=torch.uint8, device=dev), "C420", "bt470", False)


# ---------------- streaming ----------------
def _net(kind="inter", precision="fp32", large=False, seed=1024):  # (the helpers of tests/test_gpu_synth.py)
    a = types.SimpleNamespace(syn_type=kind, highres_large=large, coarse_model="HRNet", precision=precision)
    torch.manual_seed(seed)
    return (nets.InterNet if kind == "inter" else nets.ExtraNet)(a)


def _clip(B, T, H, W, seed, ignore=True):
    rng = np.random.RandomState(seed)
    frames = rng.randint(0, 256, (B, T, H, W, 3)).astype(np.uint8)
    labels = rng.randint(0, 20, (B, T, H, W)).astype(np.uint8)
    if ignore:
        labels[rng.rand(B, T, H, W) < 0.05] = 255  # Cityscapes' "ignore": an all-zero one-hot
    return frames, labels


def _per_window(syn, f, l, plan, levels):
    """the per-window interpolate results, every window after the first without its first slot"""
    parts = [syn.interpolate(f[:, t0:t1 + 1], l[:, t0:t1 + 1], levels) for t0, t1 in plan]
    return (torch.cat([p[0][:, (k > 0):] for k, p in enumerate(parts)], 1),
            torch.cat([p[1][:, (k > 0):] for k, p in enumerate(parts)], 1))


def _host_chunks(frames, labels, lengths, dev):
    """the clip as chunks of the given lengths, copied to the device one at a time"""
    t = 0
    for n in lengths:
        yield torch.from_numpy(frames[:, t:t + n]).to(dev), torch.from_numpy(labels[:, t:t + n]).to(dev)
        t += n
    assert t == frames.shape[1]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_stream_equals_the_per_window_results(dev, precision):
    B, T, H, W, levels = 2, 6, 16, 32, 2
    model = _net("inter", precision, seed=11).to(dev).eval()
    frames, labels = _clip(B, T, H, W, 21)
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    syn = VideoSynthesizer(model, max_batch=2)
    # chunks of 1, 2 and 3 frames: the first is held, then the windows are frames 0..2 and 2..5
    outs = list(syn.interpolate_stream(_host_chunks(frames, labels, [1, 2, 3], dev), levels=levels))
    assert [o[0].shape[1] for o in outs] == [9, 12]
    got_f, got_l = torch.cat([o[0] for o in outs], 1), torch.cat([o[1] for o in outs], 1)
    want_f, want_l = _per_window(VideoSynthesizer(model, max_batch=2), f, l, [(0, 2), (2, 5)], levels)
    assert got_f.shape[1] == (T - 1) * 4 + 1 == want_f.shape[1]
    assert torch.equal(got_f, want_f) and torch.equal(got_l, want_l)
    assert torch.equal(got_f[:, ::4], f) and torch.equal(got_l[:, ::4], l)  # the originals, bit for bit
    assert not torch.equal(got_f[:, 1], got_f[:, 0])  # (something was synthesised)


def test_stream_edge_cases(dev):
    model = _net("inter", "fp32", seed=11).to(dev).eval()
    syn = VideoSynthesizer(model, max_batch=2)
    frames, labels = _clip(1, 3, 16, 32, 22)
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    outs = list(syn.interpolate_stream(_host_chunks(frames, labels, [1, 1, 1], dev), levels=0))  # a pass-through
    assert torch.equal(torch.cat([o[0] for o in outs], 1), f) and torch.equal(torch.cat([o[1] for o in outs], 1), l)
    with pytest.raises(ValueError, match="at least two frames"):
        list(syn.interpolate_stream(_host_chunks(frames[:, :1], labels[:, :1], [1], dev), levels=1))
    with pytest.raises(ValueError, match="at least two frames"):
        list(syn.interpolate_stream(iter(()), levels=1))


def test_stream_equals_the_whole_clip_at_max_batch_1(dev):
    """one pair per forward in both forms: the windowing cannot change which pairs share a forward"""
    T, levels = 7, 2
    model = _net("inter", "fp32", seed=12).to(dev).eval()
    frames, labels = _clip(1, T, 16, 32, 23)
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    syn = VideoSynthesizer(model, max_batch=1)
    plan = window_plan(T, 3)
    lengths = [t1 - t0 + (k == 0) for k, (t0, t1) in enumerate(plan)]
    outs = list(syn.interpolate_stream(_host_chunks(frames, labels, lengths, dev), levels=levels))
    want_f, want_l = syn.interpolate(f, l, levels)
    assert torch.equal(torch.cat([o[0] for o in outs], 1), want_f)
    assert torch.equal(torch.cat([o[1] for o in outs], 1), want_l)


def test_device_memory_does_not_grow_with_the_clip_length(dev):
    """window 3, levels 1, the same warmed synthesiser, every yielded chunk dropped before the next is
    taken: all windows are full in both runs, so 6 windows must not peak above 2"""
    model = _net("inter", "fp32", seed=13).to(dev).eval()
    syn = VideoSynthesizer(model, max_batch=2)

    def peak(T):
        frames, labels = _clip(1, T, 16, 32, 24)
        plan = window_plan(T, 3)
        assert all(t1 - t0 == 2 for t0, t1 in plan)
        lengths = [t1 - t0 + (k == 0) for k, (t0, t1) in enumerate(plan)]
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        slots = 0
        for out_f, out_l in syn.interpolate_stream(_host_chunks(frames, labels, lengths, dev), levels=1):
            slots += out_f.shape[1]
            del out_f, out_l
        torch.cuda.synchronize(dev)
        assert slots == 2 * (T - 1) + 1
        return torch.cuda.max_memory_allocated(dev)

    peak(3)  # warm: plans, scratch
    p5, p13 = peak(5), peak(13)
    print(f"peak device memory: T=5 {p5} B, T=13 {p13} B")
    assert p13 <= p5


# ---------------- the command ----------------
def _launch_args(run, data, H, W, *extra):
    return ["--split", "test", "--syn_type", "inter", "--input_h", str(H), "--input_w", str(W), "--precision", "fp32",
            "--load_dir", str(run), "--checksession", "0", "--checkepoch", "1", "--checkpoint", "0",
            "--cycgen_load_dir", str(data), "--synth_levels", "1", *extra, "INTER", "--load_coarse"]


def test_main_launcher_streams_y4m_and_png_clips(dev, tmp_path):
    """--split test --synth_levels 1 --synth_window 3 over a C420 Y4M clip (Cmono labels) and a PNG
    clip of five 16x32 frames each; then the PNG clip with --synth_window 0; then a reader failure"""
    from PIL import Image
    from deep_video_interpolation_extrapolation_amd import main as M
    H, W, T = 16, 32, 5
    rng = np.random.RandomState(61)
    packed = rng.randint(0, 256, (T, frame_bytes(W, H, "C420"))).astype(np.uint8)
    ylab = rng.randint(0, 20, (T, H * W)).astype(np.uint8)
    frames, labels = _clip(1, T, H, W, 62, ignore=False)
    data = tmp_path / "data"
    for sub in ("rgb", "seg"):
        (data / sub / "aachen_000001").mkdir(parents=True)
    with Y4MWriter(str(data / "rgb" / "film.y4m"), W, H, (25, 1), "C420") as w:
        w.write(packed)
    with Y4MWriter(str(data / "seg" / "film.y4m"), W, H, (25, 1), "Cmono") as w:
        w.write(ylab)
    for t in range(T):
        Image.fromarray(frames[0, t]).save(data / "rgb" / "aachen_000001" / f"{t:02d}.png")
        Image.fromarray(labels[0, t]).save(data / "seg" / "aachen_000001" / f"{t:02d}.png")
    model = _net("inter", "fp32", seed=7).to(dev).eval()
    run = tmp_path / "run"
    (run / "checkpoint").mkdir(parents=True)
    torch.save({"session": 0, "epoch": 2, "coarse_model": model.coarse_model.state_dict()},
               run / "checkpoint" / "InterNet_xs2xs_inter_0_1_0.pth")
    M.main(_launch_args(run, data, H, W, "--synth_window", "3"))
    out = data / "synth"
    syn = VideoSynthesizer(model, max_batch=1)
    plan = window_plan(T, 3)

    # the Y4M clip
    d_packed = torch.from_numpy(packed).to(dev)
    f = synth.yuv_to_rgb(d_packed, H, W, "C420")[None]
    l = torch.from_numpy(ylab.reshape(1, T, H, W)).to(dev)
    want_f, want_l = _per_window(syn, f, l, plan, 1)
    r = Y4MReader(str(out / "rgb" / "film.y4m"))
    assert (r.width, r.height, r.fps, r.colourspace, r.full_range) == (W, H, (50, 1), "C420", False)
    got = r.read(100)
    r.close()
    assert got.shape == (9, packed.shape[1])
    assert np.array_equal(got[0::2], packed)  # the input's own bytes: no colour round trip
    assert np.array_equal(got[1::2], synth.rgb_to_yuv(want_f[0, 1::2], "C420", "bt601", False).cpu().numpy())
    r = Y4MReader(str(out / "seg" / "film.y4m"))
    assert (r.width, r.height, r.fps, r.colourspace) == (W, H, (50, 1), "Cmono")
    assert np.array_equal(r.read(100), want_l[0].reshape(9, H * W).cpu().numpy())
    r.close()
    r = Y4MReader(str(out / "vis_seg" / "film.y4m"))
    assert (r.width, r.height, r.fps, r.colourspace) == (W, H, (50, 1), "C444") and r.read(100).shape == (9, 3 * H * W)
    r.close()

    # the PNG clip: numbered across windows, the per-window result
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    want_f, want_l = _per_window(syn, f, l, plan, 1)

    def check_png(want_f, want_l):
        for sub in ("rgb", "seg", "vis_seg"):
            names = sorted(p.name for p in (out / sub / "aachen_000001").iterdir())
            assert names == [f"{k:04d}.png" for k in range(9)], (sub, names)
        for k in range(9):
            assert np.array_equal(np.asarray(Image.open(out / "rgb" / "aachen_000001" / f"{k:04d}.png")),
                                  want_f[0, k].cpu().numpy())
            assert np.array_equal(np.asarray(Image.open(out / "seg" / "aachen_000001" / f"{k:04d}.png")),
                                  want_l[0, k].cpu().numpy())
            assert Image.open(out / "vis_seg" / "aachen_000001" / f"{k:04d}.png").size == (W, H)

    check_png(want_f, want_l)
    shutil.rmtree(out)
    M.main(_launch_args(run, data, H, W, "--synth_window", "0"))  # today's whole-clip path
    check_png(*syn.interpolate(f, l, levels=1))
    with Y4MReader(str(out / "rgb" / "film.y4m")) as r:  # a Y4M clip is then read whole: one forward per pair
        assert np.array_equal(r.read(100), got)          # (--bs 1), so the same bytes as in windows
    shutil.rmtree(out)

    # a reader failure: a label PNG is missing from the middle of the clip -> the command ends with
    # the error (raised on its main thread) instead of hanging on a queue
    os.remove(data / "seg" / "aachen_000001" / "03.png")
    os.remove(data / "rgb" / "film.y4m")
    os.remove(data / "seg" / "film.y4m")
    child = subprocess.run([sys.executable, "-m", "deep_video_interpolation_extrapolation_amd.main"]
                           + _launch_args(run, data, H, W, "--synth_window", "3"), cwd=ROOT, capture_output=True,
                           text=True, timeout=300)
    assert child.returncode not in (0, None), child.stderr[-2000:]
    assert "FileNotFoundError" in child.stderr and "03.png" in child.stderr, child.stderr[-2000:]


def test_main_launcher_extrapolates_a_y4m_clip(dev, tmp_path):
    """EXTRA --num_pred_step 2 over a full-range C444 clip of three 16x32 frames with --synth_yuv bt709
    (and --synth_window 3, which EXTRA ignores): the two predicted frames at the input's frame rate,
    colourspace and range, every one through rgb_to_yuv"""
    from deep_video_interpolation_extrapolation_amd import main as M
    H, W, T = 16, 32, 3
    rng = np.random.RandomState(71)
    packed = rng.randint(0, 256, (T, frame_bytes(W, H, "C444"))).astype(np.uint8)
    ylab = rng.randint(0, 20, (T, H * W)).astype(np.uint8)
    data = tmp_path / "data"
    for sub in ("rgb", "seg"):
        (data / sub).mkdir(parents=True)
    with Y4MWriter(str(data / "rgb" / "film.y4m"), W, H, (30000, 1001), "C444", True) as w:
        w.write(packed)
    with Y4MWriter(str(data / "seg" / "film.y4m"), W, H, (30000, 1001), "Cmono") as w:
        w.write(ylab)
    model = _net("extra", "fp32", seed=7).to(dev).eval()
    run = tmp_path / "run"
    (run / "checkpoint").mkdir(parents=True)
    torch.save({"session": 0, "epoch": 2, "coarse_model": model.coarse_model.state_dict()},
               run / "checkpoint" / "ExtraNet_xs2xs_extra_0_1_0.pth")
    M.main(["--split", "test", "--syn_type", "extra", "--input_h", str(H), "--input_w", str(W), "--precision", "fp32",
            "--load_dir", str(run), "--checksession", "0", "--checkepoch", "1", "--checkpoint", "0",
            "--cycgen_load_dir", str(data), "--synth_yuv", "bt709", "--synth_window", "3", "EXTRA", "--load_coarse",
            "--num_pred_step", "2"])
    f = synth.yuv_to_rgb(torch.from_numpy(packed).to(dev), H, W, "C444", "bt709", True)[None]
    l = torch.from_numpy(ylab.reshape(1, T, H, W)).to(dev)
    want_f, want_l = VideoSynthesizer(model, max_batch=1).extrapolate(f[:, -2:], l[:, -2:], 2)
    out = data / "synth"
    with Y4MReader(str(out / "rgb" / "film.y4m")) as r:
        assert (r.width, r.height, r.fps, r.colourspace, r.full_range) == (W, H, (30000, 1001), "C444", True)
        assert np.array_equal(r.read(100), synth.rgb_to_yuv(want_f[0], "C444", "bt709", True).cpu().numpy())
    with Y4MReader(str(out / "seg" / "film.y4m")) as r:
        assert (r.colourspace, r.full_range) == ("Cmono", False)
        assert np.array_equal(r.read(100), want_l[0].reshape(2, H * W).cpu().numpy())
    with Y4MReader(str(out / "vis_seg" / "film.y4m")) as r:
        assert (r.colourspace, r.full_range, r.fps) == ("C444", True, (30000, 1001)) and r.read(100).shape == (2, 3 * H * W)
