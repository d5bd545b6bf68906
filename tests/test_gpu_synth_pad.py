"""GPU checks of padded-canvas synthesis (VideoSynthesizer(pad="replicate")).

* dvie_synth_load_pad / dvie_synth_finish_crop bit for bit against dvie_synth_load /
  dvie_synth_finish on index-clamped / cropped tensors (and against numpy);
* the synthesiser against the pinned oracle: pad the uint8 inputs with clamped indices in torch,
  run the aligned path (pad=None) on the canvas, crop -- byte for byte, for the coarse and the
  two-stage nets, the gather path, graph=True, the aligned size, held-out scoring and the
  `--split test --synth_pad replicate` launcher.

Every comparison is array_equal."""
import json
import types

import numpy as np
import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import nets
from deep_video_interpolation_extrapolation_amd.synth import (VideoSynthesizer, canvas_size, frame_scores, synth_finish,
                                                              synth_finish_crop, synth_load, synth_load_pad)

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 77

# (n, H, W) -> (Hp, Wp): small partial quads; both dimensions padded and W * 3 % 4 != 0; width
# only, odd W; height only; everything replicated from one pixel
SHAPES = [((2, 5, 7), (8, 8)), ((1, 13, 30), (16, 32)), ((2, 16, 29), (16, 32)), ((2, 15, 32), (16, 32)),
          ((1, 1, 1), (4, 4))]
SHAPE_IDS = ["x".join(map(str, s)) for s, _ in SHAPES]


def quantise(x):
    """the frame definition, in numpy float32 (multiply and add rounded separately, half to even)"""
    return np.rint(np.clip(x, F32(-1), F32(1)) * F32(127.5) + F32(127.5)).astype(np.uint8)


def _clamp_index(H, Hp):
    return np.minimum(np.arange(Hp), H - 1)


def _pad_np(a, H, W, Hp, Wp, hdim):
    """numpy: dimensions hdim, hdim + 1 of `a` from (H, W) to (Hp, Wp) with clamped indices"""
    return np.take(np.take(a, _clamp_index(H, Hp), axis=hdim), _clamp_index(W, Wp), axis=hdim + 1)


def _pad_t(t, Hp, Wp, hdim):
    """torch: the same on a device tensor (the oracle's padding of the uint8 inputs)"""
    H, W = t.shape[hdim], t.shape[hdim + 1]
    iy = torch.arange(Hp, device=t.device).clamp(max=H - 1)
    ix = torch.arange(Wp, device=t.device).clamp(max=W - 1)
    return t.index_select(hdim, iy).index_select(hdim + 1, ix).contiguous()


# ---------------- kernels ----------------
@pytest.mark.parametrize("shape,canvas", SHAPES, ids=SHAPE_IDS)
def test_load_pad_kernel_bit_exact(dev, shape, canvas):
    (n, H, W), (Hp, Wp) = shape, canvas
    count = n * H * W * 3
    rng = np.random.RandomState(12)
    seen = set()
    for first in ((0,) if count >= 256 else (0, 256 - count)):  # short inputs: two calls, as the load test does
        u8 = rng.permutation(np.arange(first, first + count) % 256).astype(np.uint8).reshape(n, H, W, 3)
        seen |= set(u8.ravel().tolist())
        lab = rng.randint(0, 256, (n, H, W)).astype(np.uint8)
        lab[0, H - 1, W - 1] = 255  # the corner every pad pixel of the last row / column repeats
        want_u8, want_lab = _pad_np(u8, H, W, Hp, Wp, 1), _pad_np(lab, H, W, Hp, Wp, 1)
        for ld in (8, 4):
            want = synth_load(torch.from_numpy(want_u8).to(dev), torch.full((n, Hp, Wp, ld), float("nan"), device=dev))
            out = torch.full((n, Hp, Wp, ld), float("nan"), dtype=torch.float32, device=dev)
            cbuf = torch.full((n * Hp * Wp + 2,), GUARD, dtype=torch.uint8, device=dev)
            lab_out = cbuf[1:-1].view(n, Hp, Wp)
            synth_load_pad(torch.from_numpy(u8).to(dev), torch.from_numpy(lab).to(dev), out, lab_out)
            got = out.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.cpu().numpy().view(np.uint32))
            assert not got[..., 3:].view(np.uint32).any()  # channels 3 and up: zero bits
            assert np.array_equal(lab_out.cpu().numpy(), want_lab)
            assert int(cbuf[0]) == GUARD and int(cbuf[-1]) == GUARD
            # frames alone: the label canvas is not part of the call
            out2 = torch.full_like(out, float("nan"))
            synth_load_pad(torch.from_numpy(u8).to(dev), None, out2, None)
            assert np.array_equal(out2.cpu().numpy().view(np.uint32), got.view(np.uint32))
    if count >= 210:
        assert len(seen) == 256  # all byte values occur


def _finish_inputs(n, H, W, Hp, Wp, pad_logits_nan, seed):
    """canvas rgb (padding channels and the whole pad region NaN) and logits (padding channels
    +inf; the pad region NaN or finite), with finish's half-point values and tie rows inside the
    frame and, when finite, tie rows in the pad region too"""
    rng = np.random.RandomState(seed)
    half = (((np.arange(255, dtype=np.float64) + 0.5) / 127.5) - 1.0).astype(F32)  # every half-point
    special = np.concatenate([np.array([-1, 1, -1.5, 1.5, 0], dtype=F32), half])
    count = n * H * W * 3
    if count >= special.size:
        vals = np.concatenate([special, rng.uniform(-1.2, 1.2, count - special.size).astype(F32)])
        rng.shuffle(vals)
    else:
        vals = special[rng.permutation(special.size)[:count]]
    rgb = np.full((n, Hp, Wp, 8), np.nan, dtype=F32)
    rgb[:, :H, :W, :3] = vals.reshape(n, H, W, 3)
    logits = rng.randn(n, Hp, Wp, 20).astype(F32)
    inside = np.zeros((n, Hp, Wp), dtype=bool)
    inside[:, :H, :W] = True

    def ties(where):  # the tie rows of the finish test on the first pixels of `where`, as far as they go
        rows = [([0, 19], 9.0), ([3, 7], 8.0), ([0, 5, 19], 7.5), ([4, 11, 12], 7.0), ([18, 19], 6.0),
                (list(range(20)), 0.25), (list(range(10)), -np.inf), (list(range(20)), -np.inf),
                (list(range(1, 20)), -np.inf), ([2, 19], -np.inf)]
        idx = np.argwhere(where)
        for (i, y, x), (cls, v) in zip(idx, rows):
            logits[i, y, x, cls] = v
        if len(idx):  # the last pixel as well
            i, y, x = idx[-1]
            logits[i, y, x, [17, 19]] = 5.0

    ties(inside)
    if pad_logits_nan:
        logits[~inside] = np.nan
    else:
        ties(~inside)
    seg = np.full((n, Hp, Wp, 24), np.inf, dtype=F32)  # padding channels: +inf, never compared
    seg[..., :20] = logits
    return rgb, seg


def _guarded(dev, shape, lead=1):
    """a uint8 tensor of `shape`, `lead` bytes into its allocation, guard bytes around it"""
    size = int(np.prod(shape))
    buf = torch.full((size + 2 * lead,), GUARD, dtype=torch.uint8, device=dev)
    return buf, buf[lead:lead + size].view(shape)


def _guards_intact(buf, lead=1):
    return bool((buf[:lead] == GUARD).all()) and bool((buf[-lead:] == GUARD).all())


@pytest.mark.parametrize("shape,canvas", SHAPES, ids=SHAPE_IDS)
def test_finish_crop_kernel_bit_exact(dev, shape, canvas):
    (n, H, W), (Hp, Wp) = shape, canvas
    for with_canvas in (False, True):
        rgb, seg = _finish_inputs(n, H, W, Hp, Wp, pad_logits_nan=not with_canvas, seed=11 + with_canvas)
        rgb_t, seg_t = torch.from_numpy(rgb).to(dev), torch.from_numpy(seg).to(dev)
        # dvie_synth_finish on the cropped inputs
        want_frame = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        want_label = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        synth_finish(rgb_t[:, :H, :W].contiguous(), seg_t[:, :H, :W].contiguous(), want_frame, want_label)
        want_frame, want_label = want_frame.cpu().numpy(), want_label.cpu().numpy()
        assert np.array_equal(want_frame, quantise(rgb[:, :H, :W, :3]))  # (and numpy agrees with it)
        assert np.array_equal(want_label, np.argmax(seg[:, :H, :W, :20], axis=-1).astype(np.uint8))
        # label_canvas: NULL; 1 byte into its allocation (bytewise stores); 4 bytes in (dword stores)
        for lead in ((None,) if not with_canvas else (1, 4)):
            fbuf, frame = _guarded(dev, (n, H, W, 3))
            lbuf, label = _guarded(dev, (n, H, W))
            cbuf, lcan = _guarded(dev, (n, Hp, Wp), lead) if lead else (None, None)
            synth_finish_crop(rgb_t, seg_t, frame, label, lcan)
            assert np.array_equal(frame.cpu().numpy(), want_frame)
            assert np.array_equal(label.cpu().numpy(), want_label)
            assert _guards_intact(fbuf) and _guards_intact(lbuf)
            if lead:
                want_canvas = torch.empty((n, Hp, Wp), dtype=torch.uint8, device=dev)
                synth_finish(seg=seg_t, label=want_canvas)  # dvie_synth_finish on the whole canvas
                assert np.array_equal(lcan.cpu().numpy(), want_canvas.cpu().numpy())
                assert np.array_equal(lcan.cpu().numpy(), np.argmax(seg[..., :20], axis=-1).astype(np.uint8))
                assert _guards_intact(cbuf, lead)


# ---------------- the synthesiser against the oracle ----------------
def _args(kind="inter", precision="fp32", large=False, n_scales=2, prop=False):
    return types.SimpleNamespace(syn_type=kind, highres_large=large, coarse_model="HRNet", precision=precision,
                                 n_scales=n_scales, stage3_prop=prop, refine_model="SRNRefine",
                                 stage3_model="MSResAttnRefine")


def _model(dev, name, seed=1024, **kw):
    torch.manual_seed(seed)
    return nets.__dict__[name](_args(**kw)).to(dev).eval()


def _clip(dev, B, T, H, W, seed, ignore=True):
    rng = np.random.RandomState(seed)
    frames = rng.randint(0, 256, (B, T, H, W, 3)).astype(np.uint8)
    labels = rng.randint(0, 20, (B, T, H, W)).astype(np.uint8)
    if ignore:
        labels[rng.rand(B, T, H, W) < 0.05] = 255  # Cityscapes' "ignore", also on the replicated border
        labels[:, :, H - 1, W - 1] = 255
    return torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)


def _oracle(model, f, l, call, max_batch):
    """clamp-index pad in torch -> VideoSynthesizer(pad=None) on the canvas -> crop"""
    H, W = f.shape[2:4]
    ref = VideoSynthesizer(model, max_batch=max_batch)
    Hp, Wp = canvas_size(H, W, ref.multiple)
    want_f, want_l = call(ref, _pad_t(f, Hp, Wp, 2), _pad_t(l, Hp, Wp, 2))
    assert want_f.shape[2:4] == (Hp, Wp)
    return want_f[:, :, :H, :W], want_l[:, :, :H, :W]


def _check_against_oracle(model, f, l, call, max_batch, canvas, n_out, **kw):
    B, _, H, W, _ = f.shape
    syn = VideoSynthesizer(model, max_batch=max_batch, pad="replicate", **kw)
    assert syn.canvas(H, W) == canvas != (H, W)
    got_f, got_l = call(syn, f, l)
    want_f, want_l = _oracle(model, f, l, call, max_batch)
    assert got_f.dtype == torch.uint8 and got_l.dtype == torch.uint8
    assert got_f.shape == (B, n_out, H, W, 3) and got_l.shape == (B, n_out, H, W)
    # the frame-level dimensions are contiguous (frame_scores reads them in place)
    assert got_f.stride()[2:] == (W * 3, 3, 1) and got_l.stride()[2:] == (W, 1)
    assert torch.equal(got_l, want_l)
    assert torch.equal(got_f, want_f)
    assert len({got_f[:, s].cpu().numpy().tobytes() for s in range(n_out)}) == n_out  # every slot its own frame
    return syn, got_f, got_l


# B=3 with max_batch=2: per-triple chunks in place; B=1 with max_batch=3: chunks that gather triples
@pytest.mark.parametrize("precision,B,max_batch", [("fp32", 3, 2), ("bf16", 3, 2), ("fp32", 1, 3), ("bf16", 1, 3)])
def test_interpolate_coarse_equals_oracle(dev, precision, B, max_batch):
    H, W, T, levels = 13, 30, 3, 2
    model = _model(dev, "InterNet", precision=precision)
    f, l = _clip(dev, B, T, H, W, 31)
    _, got_f, got_l = _check_against_oracle(model, f, l, lambda s, a, b: s.interpolate(a, b, levels=levels), max_batch,
                                            (16, 32), (T - 1) * 4 + 1)
    assert torch.equal(got_f[:, ::4], f) and torch.equal(got_l[:, ::4], l)  # the originals pass through


@pytest.mark.parametrize("precision,large,H,W,canvas", [("fp32", False, 16, 29, (16, 32)), ("bf16", True, 17, 33, (24, 40))],
                         ids=["16x29", "large_17x33"])
def test_extrapolate_coarse_equals_oracle(dev, precision, large, H, W, canvas):
    steps = 3
    model = _model(dev, "ExtraNet", kind="extra", precision=precision, large=large)
    f, l = _clip(dev, 3, 2, H, W, 32)
    _check_against_oracle(model, f, l, lambda s, a, b: s.extrapolate(a, b, steps=steps), 2, canvas, steps)


def test_interpolate_stage3_equals_oracle(dev):
    # B=1 with max_batch=3: the level's two triples are gathered into one forward
    H, W = 61, 126
    model = _model(dev, "InterStage3Net", precision="bf16", n_scales=2, prop=True)
    f, l = _clip(dev, 1, 3, H, W, 82)
    _, got_f, got_l = _check_against_oracle(model, f, l, lambda s, a, b: s.interpolate(a, b, levels=1), 3, (64, 128), 5)
    assert torch.equal(got_f[:, ::2], f) and torch.equal(got_l[:, ::2], l)


def test_extrapolate_refine_equals_oracle(dev):
    H, W, steps = 64, 125, 2
    model = _model(dev, "ExtraRefineNet", kind="extra", precision="fp32", n_scales=2)
    f, l = _clip(dev, 2, 2, H, W, 83)
    _check_against_oracle(model, f, l, lambda s, a, b: s.extrapolate(a, b, steps=steps), 2, (64, 128), steps)


def test_graph_replay_equals_eager(dev):
    B, H, W, steps = 2, 13, 30, 2
    model = _model(dev, "ExtraNet", kind="extra", precision="bf16")
    eager = VideoSynthesizer(model, max_batch=B, pad="replicate")
    graphed = VideoSynthesizer(model, max_batch=B, graph=True, pad="replicate")
    for seed in (41, 42):  # two different batches through the same captured graph
        f, l = _clip(dev, B, 2, H, W, seed)
        ef, el = eager.extrapolate(f, l, steps=steps)
        gf, gl = graphed.extrapolate(f, l, steps=steps)
        torch.cuda.synchronize()
        assert gf.shape == (B, steps, H, W, 3) and torch.equal(ef, gf) and torch.equal(el, gl)
        want_f, want_l = _oracle(model, f, l, lambda s, a, b: s.extrapolate(a, b, steps=steps), B)
        assert torch.equal(gf, want_f) and torch.equal(gl, want_l)
    assert len(graphed._graphs) == 1
    assert next(iter(graphed._graphs))[-2:] == (H, W)  # the key carries the cropped size
    graphed.reset()


def _traced(fn):
    """fn()'s result and the kernels the library launched meanwhile, in order"""
    lib = L.load()
    lib.dvie_trace_kernels(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = lib.dvie_traced_kernels().decode()
    finally:
        lib.dvie_trace_kernels(0)
    return out, names


def test_aligned_size_takes_the_unpadded_path(dev):
    H, W = 16, 32
    model = _model(dev, "InterNet", precision="bf16")
    f, l = _clip(dev, 2, 3, H, W, 33)
    plain, padded = VideoSynthesizer(model, max_batch=2), VideoSynthesizer(model, max_batch=2, pad="replicate")
    assert padded.canvas(H, W) == (H, W)
    (want_f, want_l), want_names = _traced(lambda: plain.interpolate(f, l, levels=1))
    (got_f, got_l), got_names = _traced(lambda: padded.interpolate(f, l, levels=1))
    assert torch.equal(got_f, want_f) and torch.equal(got_l, want_l)
    assert got_names == want_names and "synth_finish_kernel" in got_names  # the same launches
    assert "synth_load_pad" not in got_names and "synth_finish_crop" not in got_names
    # and pad=None still refuses every other size, with the text it had
    f2, l2 = _clip(dev, 1, 2, 13, 30, 34)
    with pytest.raises(ValueError, match=r"H and W must be multiples of 4, got \(13, 30\)"):
        plain.interpolate(f2, l2)
    _, names = _traced(lambda: padded.interpolate(f2, l2))
    assert "synth_load_pad_kernel" in names and "synth_finish_crop_kernel" in names


def test_score_extrapolation_at_any_size(dev):
    B, H, W, S = 2, 13, 30, 3
    model = _model(dev, "ExtraNet", kind="extra", precision="fp32")
    f, l = _clip(dev, B, 2 + S, H, W, 61)
    sc = VideoSynthesizer(model, max_batch=2, pad="replicate").score_extrapolation(f, l)
    want_f, want_l = _oracle(model, f[:, :2], l[:, :2], lambda s, a, b: s.extrapolate(a, b, steps=S), 2)
    assert torch.equal(sc.frames, want_f) and torch.equal(sc.labels, want_l)
    want = frame_scores(want_f.contiguous(), f[:, 2:], want_l.contiguous(), l[:, 2:], n_classes=20)
    assert sc.slots == [0, 1, 2] and sc.sse.shape == (B, S) and sc.scores.H == H and sc.scores.W == W
    for k in ("sse", "ssim", "agree", "valid", "inter", "uni"):
        a, b = getattr(sc, k), getattr(want, k)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), k
    assert int(sc.sse.min()) > 0
    # interpolation scores at this size too
    si = VideoSynthesizer(_model(dev, "InterNet"), max_batch=2, pad="replicate").score_interpolation(f, l, levels=1)
    assert si.slots == [1, 3] and si.frames.shape == (B, 5, H, W, 3) and torch.equal(si.frames[:, ::2], f[:, ::2])


# ---------------- the launcher ----------------
@pytest.mark.parametrize("runner,kind,name", [("INTER", "inter", "InterNet"), ("EXTRA", "extra", "ExtraNet")])
def test_main_launcher_synth_pad(dev, tmp_path, runner, kind, name):
    """--split test --synth_pad replicate over a directory with a 13x30 and a 16x32 clip of three
    PNG frames: the PNGs have the clips' own sizes and decode to the synthesiser's arrays; with
    --synth_eval it writes scores.json with the API's numbers; without the flag it raises, and
    the message names the flag."""
    from PIL import Image
    from deep_video_interpolation_extrapolation_amd import main as M
    clips = {"aachen_000001": (13, 30), "bochum_000002": (16, 32)}
    data = tmp_path / "data"
    arrays = {}
    for seed, (clip, (H, W)) in enumerate(clips.items()):
        f, l = _clip(dev, 1, 3, H, W, 51 + seed, ignore=False)
        arrays[clip] = (f, l)
        for sub, arr in (("rgb", f), ("seg", l)):
            (data / sub / clip).mkdir(parents=True)
            for t in range(3):
                Image.fromarray(arr[0, t].cpu().numpy()).save(data / sub / clip / f"{t:02d}.png")
    model = _model(dev, name, seed=7, kind=kind)
    run = tmp_path / "run"
    (run / "checkpoint").mkdir(parents=True)
    torch.save({"session": 0, "epoch": 2, "coarse_model": model.coarse_model.state_dict()},
               run / "checkpoint" / f"{name}_xs2xs_{kind}_0_1_0.pth")
    n_out = 5 if runner == "INTER" else 2

    def launch(*flags):
        M.main(["--split", "test", "--syn_type", kind, "--input_h", "16", "--input_w", "32", "--precision", "fp32",
                "--load_dir", str(run), "--checksession", "0", "--checkepoch", "1", "--checkpoint", "0",
                "--cycgen_load_dir", str(data)] + list(flags) + [runner, "--load_coarse"]
               + (["--num_pred_step", "2"] if runner == "EXTRA" else []))

    with pytest.raises(ValueError, match="multiples of 4.*--synth_pad replicate"):
        launch()
    with pytest.raises(ValueError, match="--synth_pad"):
        launch("--synth_pad", "none", "--synth_eval")
    launch("--synth_pad", "replicate")
    syn = VideoSynthesizer(model, max_batch=1, pad="replicate")
    for clip, (H, W) in clips.items():
        f, l = arrays[clip]
        want_f, want_l = syn.interpolate(f, l, levels=1) if runner == "INTER" else syn.extrapolate(f[:, -2:], l[:, -2:], 2)
        want_f, want_l = want_f[0].cpu().numpy(), want_l[0].cpu().numpy()
        assert want_f.shape == (n_out, H, W, 3)
        for sub in ("rgb", "seg", "vis_seg"):
            names = sorted(p.name for p in (data / "synth" / sub / clip).iterdir())
            assert names == [f"{k:04d}.png" for k in range(n_out)], (runner, sub, names)
        for k in range(n_out):
            assert np.array_equal(np.asarray(Image.open(data / "synth" / "rgb" / clip / f"{k:04d}.png")), want_f[k])
            assert np.array_equal(np.asarray(Image.open(data / "synth" / "seg" / clip / f"{k:04d}.png")), want_l[k])
            assert Image.open(data / "synth" / "vis_seg" / clip / f"{k:04d}.png").size == (W, H)
    launch("--synth_pad", "replicate", "--synth_eval")
    got = json.loads((data / "synth_eval" / "scores.json").read_text())
    assert sorted(got["clips"]) == sorted(clips)
    for clip in clips:
        f, l = arrays[clip]
        sc = syn.score_interpolation(f, l, levels=1) if runner == "INTER" else syn.score_extrapolation(f, l)
        assert got["clips"][clip]["slots"] == sc.slots
        for k in ("psnr", "ssim", "acc", "miou"):
            assert got["clips"][clip][k] == getattr(sc, k)[0].cpu().numpy().tolist(), (clip, k)
