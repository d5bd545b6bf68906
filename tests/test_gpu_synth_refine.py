"""GPU checks of two-stage video synthesis: dvie_synth_bridge bit for bit against the glue it
replaces, the inference plans of SRNRefine / MSResAttnRefine bitwise against the modules' eval
forward, VideoSynthesizer with the two-stage nets against a rollout composed from net(x, seg=...),
the captured graph against eager, and the `--split test` launcher."""
import types

import numpy as np
import pytest
import torch

from deep_video_interpolation_extrapolation_amd import nets
from deep_video_interpolation_extrapolation_amd.nets.InterGANNet import channel_softmax
from deep_video_interpolation_extrapolation_amd.synth import (VideoSynthesizer, midpoint_schedule, synth_bridge,
                                                              synth_load)

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = 77.0  # finite, exact in bf16, outside [-1, 1] and [0, 1]


def quantise(x):
    """the frame definition, in numpy float32 (multiply and add rounded separately, half to even)"""
    return np.rint(np.clip(x, F32(-1), F32(1)) * F32(127.5) + F32(127.5)).astype(np.uint8)


def normalise(u8):
    return ((u8.astype(F32) / F32(255)) - F32(0.5)) / F32(0.5)


def onehot(lab):
    """fp32 (.., 20, H, W) one-hot of a uint8 (.., H, W) label map; zero where the label is >= 20"""
    return (lab[..., None, :, :] == np.arange(20, dtype=np.uint8)[:, None, None]).astype(F32)


def _bits(t):
    """the raw bits of an fp32 / bf16 tensor, as an integer numpy array"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _clip(B, T, H, W, seed, ignore=True):
    rng = np.random.RandomState(seed)
    frames = rng.randint(0, 256, (B, T, H, W, 3)).astype(np.uint8)
    labels = rng.randint(0, 20, (B, T, H, W)).astype(np.uint8)
    if ignore:
        labels[rng.rand(B, T, H, W) < 0.05] = 255  # Cityscapes' "ignore": an all-zero one-hot
    return frames, labels


# ---------------- the bridge kernel ----------------
def _bridge_inputs(n, H, W):
    rng = np.random.RandomState(61)
    npix = n * H * W
    vals = rng.uniform(-1.6, 1.6, (npix, 3)).astype(F32)
    vals[0], vals[1], vals[2], vals[3] = (1, -1, 0), (1.5, -1.5, 1), (-1, 2.5, -7), (np.nextafter(F32(1), F32(2)), 0.999, -0.0)
    rgb = np.full((npix, 8), np.nan, dtype=F32)  # padding channels: NaN, never read into a result
    rgb[:, :3] = vals
    logits = (rng.randn(npix, 20) * 3).astype(F32)
    logits[0, [0, 19]] = 9.0  # ties
    logits[1, [3, 7, 11]] = 8.0
    logits[2, :] = 0.25  # all equal
    logits[3, :] = -80.0
    logits[4] = rng.uniform(78, 82, 20)  # magnitudes around +-80
    logits[5] = rng.uniform(-82, -78, 20)
    logits[6, ::2], logits[6, 1::2] = 80.0, -80.0
    logits[7, 5] = 80.0
    logits[npix - 1, [17, 19]] = 5.0  # the last pixel (a partial block)
    seg = np.full((npix, 24), np.inf, dtype=F32)  # padding channels: +inf, never read
    seg[:, :20] = logits
    return rgb.reshape(n, H, W, 8), seg.reshape(n, H, W, 24)


# (span channels, row length, [(first channel, what)]): SRNRefine's `in_full` and MSResAttnRefine's
# `in_x`, the latter also inside a wider row, so that channels behind the span exist
_LAYOUTS = {"srn": (40, 56, [(0, "rgb"), (3, "zero5"), (8, "rgb"), (11, "zero5"), (16, "soft"), (36, "zero4")]),
            "attention": (24, 24, [(0, "rgb"), (3, "zero1"), (4, "soft")]),
            "attention_wide": (24, 32, [(0, "rgb"), (3, "zero1"), (4, "soft")])}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("layout", sorted(_LAYOUTS))
def test_bridge_kernel_bit_exact(dev, layout, dtype):
    n, H, W = 2, 5, 7  # 70 pixels: one partial block
    span, ld, parts = _LAYOUTS[layout]
    rgb_np, seg_np = _bridge_inputs(n, H, W)
    rgb, seg = torch.from_numpy(rgb_np).to(dev), torch.from_numpy(seg_np).to(dev)
    # the glue the bridge replaces, on the device: the HIP channel softmax on the NCHW view of
    # the logits, torch.clamp, a cast to the destination dtype
    soft = channel_softmax(seg.permute(0, 3, 1, 2)[:, :20]).permute(0, 2, 3, 1)
    want = {"rgb": rgb[..., :3].clamp(-1, 1).to(dtype), "soft": soft.to(dtype)}
    # guard rows before and after: nothing outside the buffer's rows is written either
    store = torch.full((n * H * W + 2, ld), SENTINEL, dtype=dtype, device=dev)
    dst = store[1:-1].view(n, H, W, ld)
    synth_bridge(rgb, seg, dst[..., :span])
    torch.cuda.synchronize()
    for c0, what in parts:
        if what.startswith("zero"):
            k = int(what[4:])
            assert not _bits(dst[..., c0:c0 + k]).any(), (layout, c0)  # +0.0 exactly
        else:
            w = want[what]
            assert np.array_equal(_bits(dst[..., c0:c0 + w.shape[-1]]), _bits(w)), (layout, what)
    assert bool((dst[..., span:] == SENTINEL).all()) and bool((store[0] == SENTINEL).all()) \
        and bool((store[-1] == SENTINEL).all())
    if dtype == torch.float32:  # sanity, not the contract: the softmax against fp64 numpy
        x = seg_np[..., :20].astype(np.float64)
        e = np.exp(x - x.max(-1, keepdims=True))
        got = dst[..., span - (24 if layout == "srn" else 20):][..., :20].cpu().numpy()
        assert np.abs(got - e / e.sum(-1, keepdims=True)).max() <= 1e-6


# ---------------- the stages' inference plans against the modules ----------------
def _args(kind="inter", precision="fp32", n_scales=2, prop=False):
    return types.SimpleNamespace(syn_type=kind, highres_large=False, coarse_model="HRNet", precision=precision,
                                 n_scales=n_scales, stage3_prop=prop, refine_model="SRNRefine",
                                 stage3_model="MSResAttnRefine")


def _stage_inputs(dev, n, H, W, seed):
    """an image beyond [-1, 1], logits, stem features, two neighbour frames (slot form) and labels"""
    rng = np.random.RandomState(seed)
    img = torch.from_numpy(np.concatenate([rng.uniform(-1.3, 1.3, (n, H, W, 3)), np.zeros((n, H, W, 5))], -1)
                           .astype(F32)).to(dev)
    logits = torch.from_numpy(np.concatenate([rng.randn(n, H, W, 20) * 2, np.zeros((n, H, W, 4))], -1).astype(F32)).to(dev)
    enc = torch.from_numpy(rng.uniform(-1, 1, (n, 14, H, W)).astype(F32)).to(dev)
    frames, labels = _clip(n, 2, H, W, seed + 1)
    slots = [synth_load(torch.from_numpy(frames[:, k].copy()).to(dev),
                        torch.empty((n, H, W, 8), dtype=torch.float32, device=dev)) for k in range(2)]
    labs = [torch.from_numpy(labels[:, k].copy()).to(dev) for k in range(2)]
    return img, logits, enc, slots, labs, labels


def _nchw(t, c):
    return t.permute(0, 3, 1, 2)[:, :c]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("n_scales", [1, 2])
def test_srn_inference_plan_equals_module(dev, precision, n_scales):
    n, H, W = 2, 32, 64
    torch.manual_seed(71)
    m = nets.SRNRefine(_args(precision=precision, n_scales=n_scales)).to(dev).eval()
    img, logits, enc, _, _, _ = _stage_inputs(dev, n, H, W, 72)
    with torch.no_grad():
        want = m(_nchw(img, 3).clamp(-1, 1), channel_softmax(_nchw(logits, 20)), enc)[-1].clamp(-10, 10)
    plan = m.infer_plan(n, H, W, dev)
    assert plan.alias and plan.arena_bytes < plan.unaliased_bytes
    got = []
    for _ in range(2):  # the second run goes through whatever the first left in the arena
        out = torch.full((n, H, W, 8), float("nan"), dtype=torch.float32, device=dev)
        synth_bridge(img, logits, plan.input_view("bridge"))
        plan.set_input("enc", enc)
        plan.set_output_nchw("pred", out.permute(0, 3, 1, 2))
        plan.run_forward()
        torch.cuda.synchronize()
        got.append(out)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    assert np.array_equal(_bits(_nchw(got[0], 3)), _bits(want))
    assert np.array_equal(_bits(got[1]), _bits(got[0]))
    assert bool((got[0][..., 3:] == 0).all())  # the slot's padding channels come out as zeros


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("prop", [False, True])
def test_attention_inference_plan_equals_module(dev, precision, prop):
    n, H, W = 2, 64, 128
    torch.manual_seed(73)
    m = nets.MSResAttnRefine(_args(precision=precision, n_scales=2, prop=prop)).to(dev).eval()
    img, logits, _, slots, labs, labels = _stage_inputs(dev, n, H, W, 74)
    with torch.no_grad():
        nimg = torch.cat([_nchw(s, 3) for s in slots], 1)
        nseg = torch.from_numpy(onehot(labels).reshape(n, 40, H, W).copy()).to(dev)
        outs, _ = m(_nchw(img, 3).clamp(-1, 1), channel_softmax(_nchw(logits, 20)), nimg, nseg)
        want = outs[-1].clamp(-10, 10)
    plan = m.infer_plan(n, H, W, dev)
    got = []
    for _ in range(2):
        out = torch.full((n, H, W, 8), float("nan"), dtype=torch.float32, device=dev)
        synth_bridge(img, logits, plan.input_view("bridge"))
        plan.set_input_parts("nimg", [_nchw(s, 3) for s in slots])
        plan.set_input_labels("nseg", labs)
        plan.set_output_nchw("out", out.permute(0, 3, 1, 2))
        plan.run_forward()
        torch.cuda.synchronize()
        got.append(out)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    assert np.array_equal(_bits(_nchw(got[0], 3)), _bits(want))
    assert np.array_equal(_bits(got[1]), _bits(got[0]))


# ---------------- the synthesiser against net(x, seg=...) ----------------
def _chunks(triples, B, max_batch):
    """the synthesiser's batching rule, restated: the (triple, clip) pairs of a level in order,
    cut into chunks of max_batch -- per triple when its clips alone fill a chunk"""
    if B >= max_batch or len(triples) == 1:
        return [[(a, b, o, i) for i in range(b0, min(B, b0 + max_batch))] for a, b, o in triples
                for b0 in range(0, B, max_batch)]
    pairs = [(a, b, o, i) for a, b, o in triples for i in range(B)]
    return [pairs[k:k + max_batch] for k in range(0, len(pairs), max_batch)]


def _reference_roll(model, dev, frames, labels, in_slots, n_slots, levels, max_batch):
    """The rollout composed from the public API: per chunk one eval call
    model(cat(frames), seg=cat(one_hot)) under no_grad; the prediction is the finest output of
    the last stage (out[-1][-1] of the refine nets, out[3][-1] of the stage-3 nets), fed
    forward raw; the label is the numpy argmax of the coarse logits.  Also returns the
    quantised COARSE image of every predicted slot."""
    B = frames.shape[0]
    raw, lab, out, coarse = {}, {}, {}, {}
    for t, s in enumerate(in_slots):
        raw[s] = normalise(frames[:, t]).transpose(0, 3, 1, 2).copy()
        lab[s], out[s] = labels[:, t].copy(), frames[:, t].copy()
    for triples in levels:
        for _, _, o in triples:
            raw[o], lab[o], out[o] = np.zeros_like(raw[0]), np.zeros_like(lab[0]), np.zeros_like(out[0])
            coarse[o] = np.zeros_like(out[0])
        for chunk in _chunks(triples, B, max_batch):
            fa, fb = (np.stack([raw[p[k]][p[3]] for p in chunk]) for k in (0, 1))
            la, lb = (np.stack([lab[p[k]][p[3]] for p in chunk]) for k in (0, 1))
            with torch.no_grad():
                x = torch.cat([torch.from_numpy(fa), torch.from_numpy(fb)], 1).to(dev)
                seg = torch.cat([torch.from_numpy(onehot(la)), torch.from_numpy(onehot(lb))], 1).to(dev)
                res = model(x, seg=seg)
                assert len(res) in (3, 5)
                rgb = (res[2] if len(res) == 3 else res[3])[-1].cpu().numpy()
                crs, logits = res[0].cpu().numpy(), res[1].cpu().numpy()
            for k, (_, _, o, i) in enumerate(chunk):
                raw[o][i] = rgb[k]  # fed forward raw: not re-quantised
                lab[o][i] = np.argmax(logits[k], axis=0).astype(np.uint8)
                out[o][i] = quantise(rgb[k]).transpose(1, 2, 0)
                coarse[o][i] = quantise(crs[k]).transpose(1, 2, 0)
    return (np.stack([out[s] for s in range(n_slots)], 1), np.stack([lab[s] for s in range(n_slots)], 1), coarse)


def _model(name, kind, precision, prop=False, seed=1024):
    torch.manual_seed(seed)
    return nets.__dict__[name](_args(kind, precision, 2, prop))


def _check_interpolate(dev, model, B, T, levels, max_batch, seed):
    H, W = 64, 128
    frames, labels = _clip(B, T, H, W, seed)
    step = 1 << levels
    n_slots = (T - 1) * step + 1
    want_f, want_l, coarse = _reference_roll(model, dev, frames, labels, [t * step for t in range(T)], n_slots,
                                             midpoint_schedule(T, levels), max_batch)
    syn = VideoSynthesizer(model, max_batch=max_batch)
    got_f, got_l = syn.interpolate(torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev), levels=levels)
    assert got_f.shape == (B, n_slots, H, W, 3) and got_l.shape == (B, n_slots, H, W)
    got_f, got_l = got_f.cpu().numpy(), got_l.cpu().numpy()
    assert np.array_equal(got_f[:, ::step], frames) and np.array_equal(got_l[:, ::step], labels)  # originals
    assert np.array_equal(got_l, want_l)
    assert np.array_equal(got_f, want_f)
    for s, c in coarse.items():  # a synthesiser that returned the coarse image would not pass
        assert not np.array_equal(c, got_f[:, s]), s


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_interpolate_refine_equals_composition(dev, precision):
    model = _model("InterRefineNet", "inter", precision).to(dev).eval()
    _check_interpolate(dev, model, B=2, T=3, levels=2, max_batch=2, seed=81)


def test_interpolate_stage3_equals_composition(dev):
    # B=1 with max_batch=3: the second level's chunk gathers several triples
    model = _model("InterStage3Net", "inter", "bf16", prop=True).to(dev).eval()
    _check_interpolate(dev, model, B=1, T=3, levels=1, max_batch=3, seed=82)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_extrapolate_stage3_equals_composition(dev, precision):
    B, H, W, steps = 3, 64, 128, 2
    model = _model("ExtraStage3Net", "extra", precision).to(dev).eval()
    frames, labels = _clip(B, 2, H, W, 83)
    want_f, want_l, coarse = _reference_roll(model, dev, frames, labels, [0, 1], 2 + steps,
                                             [[(k, k + 1, k + 2)] for k in range(steps)], 2)
    syn = VideoSynthesizer(model, max_batch=2)
    got_f, got_l = syn.extrapolate(torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev), steps=steps)
    assert got_f.shape == (B, steps, H, W, 3) and got_l.shape == (B, steps, H, W)
    got_f, got_l = got_f.cpu().numpy(), got_l.cpu().numpy()
    assert np.array_equal(got_l, want_l[:, 2:])
    assert np.array_equal(got_f, want_f[:, 2:])
    for s, c in coarse.items():
        assert not np.array_equal(c, got_f[:, s - 2]), s


def test_shape_check_follows_the_coarsest_scale(dev):
    torch.manual_seed(5)
    syn = VideoSynthesizer(nets.InterRefineNet(_args(n_scales=3)))
    f = torch.zeros((1, 2, 32, 40, 3), dtype=torch.uint8, device=dev)  # 40 is no multiple of 16
    with pytest.raises(ValueError, match="multiples of 16"):
        syn.interpolate(f, torch.zeros((1, 2, 32, 40), dtype=torch.uint8, device=dev))


def test_stage3_graph_replay_equals_eager(dev):
    B, H, W, steps = 2, 64, 128, 2
    model = _model("ExtraStage3Net", "extra", "bf16").to(dev).eval()
    eager, graphed = VideoSynthesizer(model, max_batch=B), VideoSynthesizer(model, max_batch=B, graph=True)
    for seed in (91, 92):  # two different batches through the same captured graph
        frames, labels = _clip(B, 2, H, W, seed)
        f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
        ef, el = eager.extrapolate(f, l, steps=steps)
        gf, gl = graphed.extrapolate(f, l, steps=steps)
        torch.cuda.synchronize()
        assert torch.equal(ef, gf) and torch.equal(el, gl)
    assert len(graphed._graphs) == 1 and len(next(iter(graphed._graphs.values())).plans) == 3
    graphed.reset()
    assert not graphed._graphs and not any(p.busy for p in eager._plans(B, H, W, dev))


# ---------------- the launcher ----------------
def test_main_launcher_split_test_two_stage(dev, tmp_path):
    """--split test with a seeded --refine --stage3 EXTRA model (n_scales 2) over a directory of
    three 64x128 PNG frames and label maps; the PNGs written decode to the synthesiser's arrays."""
    from PIL import Image
    from deep_video_interpolation_extrapolation_amd import main as M
    H, W, n_out = 64, 128, 2
    frames, labels = _clip(1, 3, H, W, 95, ignore=False)
    data = tmp_path / "data"
    for sub in ("rgb", "seg"):
        (data / sub / "aachen_000001").mkdir(parents=True)
    for t in range(3):
        Image.fromarray(frames[0, t]).save(data / "rgb" / "aachen_000001" / f"{t:02d}.png")
        Image.fromarray(labels[0, t]).save(data / "seg" / "aachen_000001" / f"{t:02d}.png")
    model = _model("ExtraStage3Net", "extra", "fp32", seed=7).to(dev).eval()
    run = tmp_path / "run"
    (run / "checkpoint").mkdir(parents=True)
    torch.save({"session": 0, "epoch": 2, "coarse_model": model.coarse_model.state_dict(),
                "refine_model": model.refine_model.state_dict(), "stage3_model": model.stage3_model.state_dict()},
               run / "checkpoint" / "ExtraStage3Net_xs2xs_extra_0_1_0.pth")
    M.main(["--split", "test", "--syn_type", "extra", "--input_h", str(H), "--input_w", str(W), "--precision", "fp32",
            "--load_dir", str(run), "--checksession", "0", "--checkepoch", "1", "--checkpoint", "0",
            "--cycgen_load_dir", str(data), "EXTRA", "--model", "ExtraStage3Net", "--load_model", "ExtraStage3Net",
            "--load_coarse", "--refine", "--refine_model", "SRNRefine", "--load_refine", "--stage3", "--load_stage3",
            "--n_sc", "2", "--num_pred_step", str(n_out)])
    syn = VideoSynthesizer(model, max_batch=1)
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    want_f, want_l = syn.extrapolate(f[:, -2:], l[:, -2:], n_out)
    want_f, want_l = want_f[0].cpu().numpy(), want_l[0].cpu().numpy()
    out = data / "synth"
    for sub in ("rgb", "seg", "vis_seg"):
        names = sorted(p.name for p in (out / sub / "aachen_000001").iterdir())
        assert names == [f"{k:04d}.png" for k in range(n_out)], (sub, names)
    for k in range(n_out):
        assert np.array_equal(np.asarray(Image.open(out / "rgb" / "aachen_000001" / f"{k:04d}.png")), want_f[k])
        assert np.array_equal(np.asarray(Image.open(out / "seg" / "aachen_000001" / f"{k:04d}.png")), want_l[k])
        assert Image.open(out / "vis_seg" / "aachen_000001" / f"{k:04d}.png").size == (W, H)
