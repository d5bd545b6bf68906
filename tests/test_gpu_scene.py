"""GPU checks of scene-cut detection: dvie_synth_scene and dvie_synth_cutfill against the numpy
restatement (tests/scene_ref.py), exactly; interpolate / interpolate_stream with scene= against the
plain calls and the fill rule; and the `--split test --synth_scd` command over a Y4M and a PNG clip.
The end-to-end inputs are scene_ref's clips, whose margins tests/test_scene_cpu.py asserts."""
import logging
import types

import numpy as np
import pytest
import torch

from deep_video_interpolation_extrapolation_amd import nets, synth
from deep_video_interpolation_extrapolation_amd.synth import SceneCuts, VideoSynthesizer, window_plan
from deep_video_interpolation_extrapolation_amd.video_io import Y4MReader, Y4MWriter
import scene_ref as R
import yuv_ref as Y

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 1, 1), (2, 3, 3, 5), (1, 4, 17, 33), (2, 5, 64, 96)]
SCENE = SceneCuts(mad=R.MAD, hist=R.HIST)


def _as_view(host, view, dev):
    """host (B, T, H, W, 3) on the device as a view of the named kind, holding the same frames"""
    B, T, H, W, _ = host.shape
    if view == "contiguous":
        return torch.from_numpy(host).to(dev)
    if view == "every_other":  # [:, ::2] of a clip of 2T - 1 frames; the frames between are noise
        big = np.random.RandomState(5).randint(0, 256, (B, 2 * T - 1, H, W, 3)).astype(np.uint8)
        big[:, ::2] = host
        return torch.from_numpy(big).to(dev)[:, ::2]
    if view == "slot_major":  # the transposed view of (T, B) storage, as interpolate returns it
        return torch.from_numpy(np.ascontiguousarray(host.transpose(1, 0, 2, 3, 4))).to(dev).transpose(0, 1)
    assert view == "odd_offset"  # a slice of a larger buffer that starts at an odd byte
    flat = torch.full((host.size + 8,), 0x5A, dtype=torch.uint8, device=dev)
    flat[3:3 + host.size] = torch.from_numpy(host.reshape(-1)).to(dev)
    return flat[3:3 + host.size].view(B, T, H, W, 3)


# ---------------- the statistic ----------------
@pytest.mark.parametrize("view", ["contiguous", "every_other", "slot_major", "odd_offset"])
@pytest.mark.parametrize("B,T,H,W", SHAPES)
def test_statistic_equals_the_reference(dev, B, T, H, W, view):
    host = np.random.RandomState(1000 * H + W + T).randint(0, 256, (B, T, H, W, 3)).astype(np.uint8)
    frames = _as_view(host, view, dev)
    assert tuple(frames.shape) == host.shape
    sad, hdiff = synth.scene_stats(frames)
    assert sad.dtype == hdiff.dtype == torch.int64 and tuple(sad.shape) == tuple(hdiff.shape) == (B, T - 1)
    want_sad, want_hdiff = R.stats(host)
    assert np.array_equal(sad.cpu().numpy(), want_sad) and np.array_equal(hdiff.cpu().numpy(), want_hdiff)
    # the flags: limits that sit exactly on one pair's two sums, and one above each
    s, h = int(want_sad[0, 0]), int(want_hdiff[0, 0])
    n = H * W
    for mad, hist in ((s / n, h / (2 * n)), (min((s + 1) / n, 255.0), h / (2 * n)), (s / n, min((h + 1) / (2 * n), 1.0))):
        got = synth.scene_cuts(frames, mad, hist)
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), R.cuts(host, mad, hist)), (mad, hist)


def test_statistic_extremes_and_one_bin(dev):
    B, T, H, W = 2, 4, 64, 96
    host = np.empty((B, T, H, W, 3), np.uint8)
    host[0] = 137  # every frame one constant: every count in one bin
    host[1, 0::2], host[1, 1::2] = 0, 255
    sad, hdiff = synth.scene_stats(torch.from_numpy(host).to(dev))
    assert sad.cpu().tolist() == [[0] * 3, [255 * H * W] * 3] and hdiff.cpu().tolist() == [[0] * 3, [2 * H * W] * 3]
    assert np.array_equal(sad.cpu().numpy(), R.stats(host)[0]) and np.array_equal(hdiff.cpu().numpy(), R.stats(host)[1])
    cuts = synth.scene_cuts(torch.from_numpy(host).to(dev), 255, 1)  # the largest thresholds: 0 against 255 alone
    assert cuts.cpu().tolist() == [[False] * 3, [True] * 3]


def test_two_calls_give_the_same_bits(dev):
    host = np.random.RandomState(3).randint(0, 256, (2, 5, 64, 96, 3)).astype(np.uint8)
    frames = torch.from_numpy(host).to(dev)
    a, b = synth.scene_stats(frames), synth.scene_stats(frames)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(synth.scene_cuts(frames, 80, 0.1), synth.scene_cuts(frames, 80, 0.1))


# ---------------- the fill ----------------
@pytest.mark.parametrize("nbytes", [1, 15, 1683])
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_cut_fill_equals_the_reference(dev, levels, nbytes):
    B, T = 2, 4
    S = (T - 1) * (1 << levels) + 1
    rng = np.random.RandomState(10 * levels + nbytes)
    store = rng.randint(0, 256, (S, B, nbytes)).astype(np.uint8)  # slot-major storage
    host = store.transpose(1, 0, 2)
    for flags in ([[0, 0, 0], [0, 0, 0]], [[1, 1, 1], [1, 1, 1]], [[1, 0, 1], [0, 1, 0]]):
        flags = np.array(flags, dtype=bool)
        want = R.fill(host, flags, levels)
        d_flags = torch.from_numpy(flags).to(dev)
        # the transposed slot-major view, in place
        d_store = torch.from_numpy(store).to(dev)
        view = d_store.transpose(0, 1)
        assert synth.cut_fill(view, d_flags, levels) is view
        got = d_store.cpu().numpy().transpose(1, 0, 2)
        assert np.array_equal(got, want), flags
        step = 1 << levels
        assert np.array_equal(got[:, ::step], host[:, ::step])  # input slots
        for b in range(B):
            for t in range(T - 1):
                if not flags[b, t]:
                    assert np.array_equal(got[b, t * step:(t + 1) * step + 1], host[b, t * step:(t + 1) * step + 1])
        # a contiguous (B, S, n) tensor at an odd byte offset, uint8 flags
        flat = torch.full((host.size + 8,), 0x5A, dtype=torch.uint8, device=dev)
        flat[3:3 + host.size] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1)).to(dev)
        synth.cut_fill(flat[3:3 + host.size].view(B, S, nbytes), d_flags.to(torch.uint8), levels)
        out = flat.cpu().numpy()
        assert np.array_equal(out[3:3 + host.size].reshape(B, S, nbytes), want)
        assert (out[:3] == 0x5A).all() and (out[3 + host.size:] == 0x5A).all()


def test_cut_fill_levels_0_and_shape_checks(dev):
    slots = torch.arange(2 * 4 * 6, dtype=torch.uint8, device=dev).view(2, 4, 6)
    flags = torch.ones((2, 3), dtype=torch.bool, device=dev)
    before = slots.clone()
    synth.cut_fill(slots, flags, 0)
    assert torch.equal(slots, before)
    with pytest.raises(ValueError):
        synth.cut_fill(slots, flags, 1)  # 4 slots are not 3 pairs at levels 1
    with pytest.raises(ValueError):
        synth.cut_fill(slots, flags[:1], 0)


# ---------------- interpolate ----------------
def _net(kind="inter", precision="fp32", large=False, seed=1024):  # (the helpers of tests/test_gpu_stream.py)
    a = types.SimpleNamespace(syn_type=kind, highres_large=large, coarse_model="HRNet", precision=precision)
    torch.manual_seed(seed)
    return (nets.InterNet if kind == "inter" else nets.ExtraNet)(a)


def _host_chunks(frames, labels, lengths, dev):
    """the clip as chunks of the given lengths, copied to the device one at a time"""
    t = 0
    for n in lengths:
        yield torch.from_numpy(frames[:, t:t + n]).to(dev), torch.from_numpy(labels[:, t:t + n]).to(dev)
        t += n
    assert t == frames.shape[1]


def _per_window(syn, f, l, plan, levels, scene=None):
    """the per-window interpolate results, every window after the first without its first slot;
    with scene also the windows' flags side by side"""
    parts = [syn.interpolate(f[:, t0:t1 + 1], l[:, t0:t1 + 1], levels, scene) for t0, t1 in plan]
    out = (torch.cat([p[0][:, (k > 0):] for k, p in enumerate(parts)], 1),
           torch.cat([p[1][:, (k > 0):] for k, p in enumerate(parts)], 1))
    return out + ((torch.cat([p[2] for p in parts], 1),) if scene is not None else ())


@pytest.fixture(scope="module")
def model(dev):
    return _net("inter", "fp32", seed=11).to(dev).eval()


@pytest.mark.parametrize("H,W,pad", [(16, 32, None), (15, 30, "replicate")])
def test_interpolate_holds_frames_across_the_cut(dev, model, H, W, pad):
    levels, step = 2, 4
    frames, labels = R.api_clips(H, W)
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    syn = VideoSynthesizer(model, max_batch=2, pad=pad)
    plain = syn.interpolate(f, l, levels)
    assert len(plain) == 2
    plain_f, plain_l = plain[0].cpu().numpy(), plain[1].cpu().numpy()
    out_f, out_l, cuts = syn.interpolate(f, l, levels, scene=SCENE)
    want = R.cuts(frames, R.MAD, R.HIST)
    assert want.tolist() == [[False, True, False], [False] * 3]
    assert cuts.dtype == torch.bool and np.array_equal(cuts.cpu().numpy(), want)
    got_f, got_l = out_f.cpu().numpy(), out_l.cpu().numpy()
    assert got_f.shape == (2, 13, H, W, 3) and got_l.shape == (2, 13, H, W)
    # every segment of clip 1 and the unflagged segments of clip 0: the plain call, byte for byte
    assert np.array_equal(got_f[1], plain_f[1]) and np.array_equal(got_l[1], plain_l[1])
    for seg in (slice(0, 5), slice(8, 13)):
        assert np.array_equal(got_f[0, seg], plain_f[0, seg]) and np.array_equal(got_l[0, seg], plain_l[0, seg])
    # the flagged segment: slots 5, 6 hold input frame 1, slot 7 input frame 2
    for slot, t in ((5, 1), (6, 1), (7, 2)):
        assert np.array_equal(got_f[0, slot], frames[0, t]) and np.array_equal(got_l[0, slot], labels[0, t])
        assert not np.array_equal(plain_f[0, slot], frames[0, t])  # (the plain call blends there)
    assert np.array_equal(got_f, R.fill(plain_f, want, levels)) and np.array_equal(got_l, R.fill(plain_l, want, levels))
    assert np.array_equal(got_f[:, ::step], frames) and np.array_equal(got_l[:, ::step], labels)
    # thresholds nothing reaches: the plain call
    out_f, out_l, cuts = syn.interpolate(f, l, levels, scene=SceneCuts(mad=255, hist=1))
    assert not cuts.any() and np.array_equal(out_f.cpu().numpy(), plain_f) and np.array_equal(out_l.cpu().numpy(), plain_l)


def test_interpolate_levels_0_returns_the_flags(dev, model):
    frames, labels = R.api_clips()
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    out_f, out_l, cuts = VideoSynthesizer(model, max_batch=2).interpolate(f, l, 0, scene=SCENE)
    assert torch.equal(out_f, f) and torch.equal(out_l, l)
    assert cuts.cpu().tolist() == [[False, True, False], [False] * 3]
    with pytest.raises(ValueError, match="SceneCuts"):
        VideoSynthesizer(model, max_batch=2).interpolate(f, l, 1, scene=(40, 0.3))


def test_stream_equals_the_per_window_results_with_the_cut_on_a_boundary(dev, model):
    """windows 0..2 and 2..4, the cut between frames 2 and 3: the carried frame is its left side"""
    levels = 2
    frames, labels = R.api_clips(16, 32, T=5, cut_at=3)
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    syn = VideoSynthesizer(model, max_batch=2)
    outs = list(syn.interpolate_stream(_host_chunks(frames, labels, [1, 2, 2], dev), levels=levels, scene=SCENE))
    assert [len(o) for o in outs] == [3, 3] and [o[0].shape[1] for o in outs] == [9, 8]
    assert [tuple(o[2].shape) for o in outs] == [(2, 2), (2, 2)]
    got = [torch.cat([o[k] for o in outs], 1) for k in range(3)]
    want = _per_window(VideoSynthesizer(model, max_batch=2), f, l, [(0, 2), (2, 4)], levels, SCENE)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    assert got[2].cpu().tolist() == [[False, False, True, False], [False] * 4]
    for slot, t in ((9, 2), (10, 2), (11, 3)):  # held: the carried frame twice, then frame 3
        assert torch.equal(got[0][0, slot], f[0, t]) and torch.equal(got[1][0, slot], l[0, t])
    plain = _per_window(syn, f, l, [(0, 2), (2, 4)], levels)
    assert np.array_equal(got[0].cpu().numpy(), R.fill(plain[0].cpu().numpy(), got[2].cpu().numpy(), levels))
    # without scene the generator yields pairs, as before
    assert all(len(o) == 2 for o in syn.interpolate_stream(_host_chunks(frames, labels, [1, 2, 2], dev), levels=1))


def test_stream_equals_the_whole_clip_at_max_batch_1(dev, model):
    levels = 2
    frames, labels = (x[:1] for x in R.api_clips(16, 32, T=5, cut_at=3))
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    syn = VideoSynthesizer(model, max_batch=1)
    outs = list(syn.interpolate_stream(_host_chunks(frames, labels, [3, 2], dev), levels=levels, scene=SCENE))
    want = syn.interpolate(f, l, levels, scene=SCENE)
    for k in range(3):
        assert torch.equal(torch.cat([o[k] for o in outs], 1), want[k]), k
    assert want[2].cpu().tolist() == [[False, False, True, False]]


# ---------------- the command ----------------
def _launch_args(run, data, H, W, *extra):
    return ["--split", "test", "--syn_type", "inter", "--input_h", str(H), "--input_w", str(W), "--precision", "fp32",
            "--load_dir", str(run), "--checksession", "0", "--checkepoch", "1", "--checkpoint", "0",
            "--cycgen_load_dir", str(data), "--synth_levels", "2", "--synth_window", "3", *extra, "INTER", "--load_coarse"]


def test_main_launcher_holds_frames_in_y4m_and_png_clips(dev, tmp_path, caplog):
    """--synth_levels 2 --synth_window 3 --synth_scd over a C420 Y4M clip and a PNG clip of five 16x32
    frames with a cut between frames 2 and 3 (the boundary of the two windows); then without the flag"""
    import shutil
    from PIL import Image
    from deep_video_interpolation_extrapolation_amd import main as M
    H, W, T, levels, step = 16, 32, 5, 2, 4
    frames, labels = R.command_clip(H, W, T)
    packed = Y.rgb2yuv_int(frames[0], "C420")
    data = tmp_path / "data"
    for sub in ("rgb", "seg"):
        (data / sub / "aachen_000001").mkdir(parents=True)
    with Y4MWriter(str(data / "rgb" / "film.y4m"), W, H, (25, 1), "C420") as w:
        w.write(packed)
    with Y4MWriter(str(data / "seg" / "film.y4m"), W, H, (25, 1), "Cmono") as w:
        w.write(labels[0].reshape(T, H * W))
    for t in range(T):
        Image.fromarray(frames[0, t]).save(data / "rgb" / "aachen_000001" / f"{t:02d}.png")
        Image.fromarray(labels[0, t]).save(data / "seg" / "aachen_000001" / f"{t:02d}.png")
    net = _net("inter", "fp32", seed=7).to(dev).eval()
    run = tmp_path / "run"
    (run / "checkpoint").mkdir(parents=True)
    torch.save({"session": 0, "epoch": 2, "coarse_model": net.coarse_model.state_dict()},
               run / "checkpoint" / "InterNet_xs2xs_inter_0_1_0.pth")
    syn = VideoSynthesizer(net, max_batch=1)
    plan = window_plan(T, 3)
    out = data / "synth"
    S = (T - 1) * step + 1
    held = {9: 2, 10: 2, 11: 3}  # output slot -> the input frame it holds

    def read(sub):
        with Y4MReader(str(out / sub / "film.y4m")) as r:
            return r.read(100)

    def check_png(want_f, want_l):
        for k in range(S):
            assert np.array_equal(np.asarray(Image.open(out / "rgb" / "aachen_000001" / f"{k:04d}.png")),
                                  want_f[0, k].cpu().numpy()), k
            assert np.array_equal(np.asarray(Image.open(out / "seg" / "aachen_000001" / f"{k:04d}.png")),
                                  want_l[0, k].cpu().numpy()), k

    fy = synth.yuv_to_rgb(torch.from_numpy(packed).to(dev), H, W, "C420")[None]
    ly = torch.from_numpy(labels).to(dev)
    fp = torch.from_numpy(frames).to(dev)

    with caplog.at_level(logging.INFO):
        M.main(_launch_args(run, data, H, W, "--synth_scd", "--synth_scd_mad", "40", "--synth_scd_hist", "0.3"))
    assert "film: 1 scene cut after input frame [2]" in caplog.text
    assert "aachen_000001: 1 scene cut after input frame [2]" in caplog.text
    want_f, want_l, cuts = _per_window(syn, fy, ly, plan, levels, SCENE)
    assert cuts.cpu().tolist() == [[False, False, True, False]]
    got = read("rgb")
    assert got.shape == (S, packed.shape[1])
    assert np.array_equal(got[0::step], packed)  # the inputs' own bytes
    for k, t in held.items():  # the held slots too: no colour round trip
        assert np.array_equal(got[k], packed[t]), k
    blend = [k for k in range(S) if k % step and k not in held]
    assert np.array_equal(got[blend], synth.rgb_to_yuv(want_f[0, blend], "C420", "bt601", False).cpu().numpy())
    got_l = read("seg")
    assert np.array_equal(got_l, want_l[0].reshape(S, H * W).cpu().numpy())
    for k, t in held.items():
        assert np.array_equal(got_l[k], labels[0, t].reshape(-1))
    assert read("vis_seg").shape == (S, 3 * H * W)
    want_f, want_l, cuts = _per_window(syn, fp, ly, plan, levels, SCENE)
    check_png(want_f, want_l)
    for k, t in held.items():
        assert torch.equal(want_f[0, k], fp[0, t])
    shutil.rmtree(out)

    # without --synth_scd: the plain per-window results, every synthesised slot through rgb_to_yuv
    caplog.clear()
    with caplog.at_level(logging.INFO):
        M.main(_launch_args(run, data, H, W))
    assert "scene cut" not in caplog.text
    want_f, want_l = _per_window(syn, fy, ly, plan, levels)
    got = read("rgb")
    assert np.array_equal(got[0::step], packed)
    synthd = [k for k in range(S) if k % step]
    assert np.array_equal(got[synthd], synth.rgb_to_yuv(want_f[0, synthd], "C420", "bt601", False).cpu().numpy())
    assert not np.array_equal(got[9], packed[2])
    assert np.array_equal(read("seg"), want_l[0].reshape(S, H * W).cpu().numpy())
    check_png(*_per_window(syn, fp, ly, plan, levels))
