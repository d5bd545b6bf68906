"""GPU checks of the self-ensemble (VideoSynthesizer(ensemble=), dvie_synth_flip, dvie_synth_ens_acc).

* the two kernels against numpy, bit for bit, with guard bytes around every output;
* the synthesiser against a composition from the public module call: per chunk and member one
  model(x, seg=seg) on inputs swapped or mirrored with numpy, the outputs mirrored back, the fp32
  mean (((x0 + x1) + x2) + x3) * (1 / M) in member order, the mean fed forward raw;
* the two symmetries an ensemble buys, through the public API;
* the ensemble under the padded canvas, tiles, graph replay, streaming, scoring and the launcher.

Every comparison is byte-exact; no tolerance is used anywhere."""
import json
import logging
import types

import numpy as np
import pytest
import torch

import tile_ref as R
from deep_video_interpolation_extrapolation_amd import nets
from deep_video_interpolation_extrapolation_amd.synth import (VideoSynthesizer, ensemble_members, midpoint_schedule,
                                                              synth_ens_acc, synth_flip, synth_load)

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 77


def quantise(x):
    """the frame definition, in numpy float32 (multiply and add rounded separately, half to even)"""
    return np.rint(np.clip(x, F32(-1), F32(1)) * F32(127.5) + F32(127.5)).astype(np.uint8)


def normalise(u8):
    return ((u8.astype(F32) / F32(255)) - F32(0.5)) / F32(0.5)


def onehot(lab):
    """fp32 (.., 20, H, W) one-hot of a uint8 (.., H, W) label map; zero where the label is >= 20"""
    return (lab[..., None, :, :] == np.arange(20, dtype=np.uint8)[:, None, None]).astype(F32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------- the kernels ----------------
@pytest.mark.parametrize("soff,doff", [(0, 0), (1, 0), (1, 3)])
@pytest.mark.parametrize("H,W", [(3, 1), (3, 2), (3, 5), (3, 8), (3, 13), (1, 13)])
def test_flip_kernel_bit_exact(dev, H, W, soff, doff):
    """sources that are views strided over n (every second image of a larger block); the label
    source at byte offset `soff` into its buffer and the label destination at `doff` into its own
    (0: the dword path where the width allows it; odd: every byte on its own)"""
    n, ld = 2, 8
    rng = np.random.RandomState(100 * W + 10 * H + soff)
    big = rng.randn(2 * n, H, W, ld).astype(F32)
    lbig = rng.randint(0, 256, (2 * n, H, W)).astype(np.uint8)
    src = torch.from_numpy(big).to(dev)[::2]
    lbuf = torch.full((soff + lbig.size + 5,), GUARD, dtype=torch.uint8, device=dev)
    lbuf[soff:soff + lbig.size] = torch.from_numpy(lbig.reshape(-1)).to(dev)
    lsrc = lbuf[soff:soff + lbig.size].view(2 * n, H, W)[::2]
    assert not src.is_contiguous() and lsrc.data_ptr() % 4 == soff % 4
    dbuf = torch.full((n * H * W * ld + 2 * 16,), float(GUARD), dtype=torch.float32, device=dev)
    dst = dbuf[16:16 + n * H * W * ld].view(n, H, W, ld)
    lo = 16 + doff
    ldbuf = torch.full((lo + n * H * W + 16,), GUARD, dtype=torch.uint8, device=dev)
    ldst = ldbuf[lo:lo + n * H * W].view(n, H, W)
    synth_flip(src, lsrc, dst, ldst)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dst.cpu().numpy()), _bits(big[::2, :, ::-1]))
    assert np.array_equal(ldst.cpu().numpy(), lbig[::2, :, ::-1])
    d, ldn = dbuf.cpu().numpy(), ldbuf.cpu().numpy()
    assert (d[:16] == GUARD).all() and (d[-16:] == GUARD).all()  # nothing outside the outputs is written
    assert (ldn[:lo] == GUARD).all() and (ldn[-16:] == GUARD).all()
    assert np.array_equal(lbuf.cpu().numpy()[soff:soff + lbig.size], lbig.reshape(-1))  # the sources are only read
    # the images alone
    dst.fill_(0)
    synth_flip(src, None, dst, None)
    assert np.array_equal(_bits(dst.cpu().numpy()), _bits(big[::2, :, ::-1]))


@pytest.mark.parametrize("direct", [False, True], ids=["first", "bound"])
@pytest.mark.parametrize("setting", ["time", "flip", "time+flip"])
def test_ens_acc_kernel_bit_exact(dev, setting, direct):
    """chains of two and of four members with the flip pattern of every setting; member 0 through a
    `first` call, or already in the accumulators (what a forward bound to them leaves, padding
    channels of anything); 15 pixels: vectors and a tail of the 256-lane blocks' last one"""
    n, H, W = 2, 3, 5
    members = ensemble_members(setting)
    M = len(members)
    rng = np.random.RandomState(7 + M)
    xs = [(rng.randn(n, H, W, 8).astype(F32), rng.randn(n, H, W, 24).astype(F32)) for _ in members]  # (padding: anything)
    nr, ns = n * H * W * 8, n * H * W * 24
    buf = torch.full((nr + ns + 64,), float(GUARD), dtype=torch.float32, device=dev)  # [rgb_acc | seg_acc | guard]
    rgb_acc, seg_acc = buf[:nr].view(n, H, W, 8), buf[nr:nr + ns].view(n, H, W, 24)
    want_r = want_s = None
    for m, ((_, flip), (r, s)) in enumerate(zip(members, xs)):
        tr, ts = torch.from_numpy(r).to(dev), torch.from_numpy(s).to(dev)
        if m == 0 and direct:
            rgb_acc.copy_(tr)
            seg_acc.copy_(ts)
        else:
            synth_ens_acc(tr, ts, rgb_acc, seg_acc, flip=flip, first=m == 0, last_m=M if m == M - 1 else 0)
        r, s = (r[:, :, ::-1], s[:, :, ::-1]) if flip else (r, s)
        want_r = r[..., :3] if m == 0 else want_r + r[..., :3]
        want_s = s[..., :20] if m == 0 else want_s + s[..., :20]
        assert want_r.dtype == F32 and want_s.dtype == F32
    want_r, want_s = want_r * F32(1 / M), want_s * F32(1 / M)
    torch.cuda.synchronize()
    got_r, got_s, tail = rgb_acc.cpu().numpy(), seg_acc.cpu().numpy(), buf[nr + ns:].cpu().numpy()
    assert np.array_equal(_bits(got_r[..., :3]), _bits(want_r)) and np.array_equal(_bits(got_s[..., :20]), _bits(want_s))
    assert (_bits(got_r[..., 3:]) == 0).all() and (_bits(got_s[..., 20:]) == 0).all()  # the padding channels: +0
    assert (tail == GUARD).all()  # what lies after the accumulators is untouched


# ---------------- the synthesiser against the public module call ----------------
def _args(kind="inter", precision="fp32", n_scales=2, prop=False):
    return types.SimpleNamespace(syn_type=kind, highres_large=False, coarse_model="HRNet", precision=precision,
                                 n_scales=n_scales, stage3_prop=prop, refine_model="SRNRefine",
                                 stage3_model="MSResAttnRefine")


def _model(dev, name, kind="inter", precision="fp32", prop=False, seed=1024):
    torch.manual_seed(seed)
    return nets.__dict__[name](_args(kind, precision, 2, prop)).to(dev).eval()


def _clip(B, T, H, W, seed, ignore=True):
    rng = np.random.RandomState(seed)
    frames = rng.randint(0, 256, (B, T, H, W, 3)).astype(np.uint8)
    labels = rng.randint(0, 20, (B, T, H, W)).astype(np.uint8)
    if ignore:
        labels[rng.rand(B, T, H, W) < 0.05] = 255  # Cityscapes' "ignore": an all-zero one-hot
    return frames, labels


def _dev(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def _chunks(triples, B, max_batch):
    """the synthesiser's batching rule, restated: the (triple, clip) pairs of a level in order,
    cut into chunks of max_batch -- per triple when its clips alone fill a chunk"""
    if B >= max_batch or len(triples) == 1:
        return [[(a, b, o, i) for i in range(b0, min(B, b0 + max_batch))] for a, b, o in triples
                for b0 in range(0, B, max_batch)]
    pairs = [(a, b, o, i) for a, b, o in triples for i in range(B)]
    return [pairs[k:k + max_batch] for k in range(0, len(pairs), max_batch)]


def _member_forward(model, dev, fa, fb, la, lb, swap, flip):
    """one member from the public call: raw frames (n, 3, H, W) and label maps (n, H, W), exchanged
    and / or mirrored along W with numpy -> (image, coarse logits) mirrored back, as numpy; the
    image is the finest output of the last stage"""
    if swap:
        fa, fb, la, lb = fb, fa, lb, la
    if flip:
        fa, fb, la, lb = (np.ascontiguousarray(t[..., ::-1]) for t in (fa, fb, la, lb))
    with torch.no_grad():
        x = torch.cat([torch.from_numpy(fa), torch.from_numpy(fb)], 1).to(dev)
        seg = torch.cat([torch.from_numpy(onehot(la)), torch.from_numpy(onehot(lb))], 1).to(dev)
        res = model(x, seg=seg)
        assert len(res) in (2, 3, 5)
        rgb = res[0] if len(res) == 2 else (res[2] if len(res) == 3 else res[3])[-1]
        rgb, logits = rgb.cpu().numpy(), res[1].cpu().numpy()
    assert rgb.dtype == F32 and logits.dtype == F32
    return (rgb[..., ::-1], logits[..., ::-1]) if flip else (rgb, logits)


def _reference_roll(model, dev, frames, labels, in_slots, n_slots, levels, max_batch, setting):
    """The rollout composed from the public API: per chunk and member one eval call; the fp32 mean
    of the members in their order; the mean fed forward raw, with the numpy argmax of the mean
    logits; the frame is the quantised mean."""
    members = ensemble_members(setting)
    M = len(members)
    B = frames.shape[0]
    raw, lab, out = {}, {}, {}
    for t, s in enumerate(in_slots):
        raw[s] = normalise(frames[:, t]).transpose(0, 3, 1, 2).copy()
        lab[s], out[s] = labels[:, t].copy(), frames[:, t].copy()
    for triples in levels:
        for _, _, o in triples:
            raw[o], lab[o], out[o] = np.zeros_like(raw[0]), np.zeros_like(lab[0]), np.zeros_like(out[0])
        for chunk in _chunks(triples, B, max_batch):
            fa, fb = (np.stack([raw[p[k]][p[3]] for p in chunk]) for k in (0, 1))
            la, lb = (np.stack([lab[p[k]][p[3]] for p in chunk]) for k in (0, 1))
            rgb = logits = None
            for m, (swap, flip) in enumerate(members):
                r, s = _member_forward(model, dev, fa, fb, la, lb, swap, flip)
                rgb, logits = (r, s) if m == 0 else (rgb + r, logits + s)
            if M > 1:
                rgb, logits = rgb * F32(1 / M), logits * F32(1 / M)
            assert rgb.dtype == F32 and logits.dtype == F32
            for k, (_, _, o, i) in enumerate(chunk):
                raw[o][i] = rgb[k]  # fed forward raw: unclamped, not re-quantised
                lab[o][i] = np.argmax(logits[k], axis=0).astype(np.uint8)
                out[o][i] = quantise(rgb[k]).transpose(1, 2, 0)
    return np.stack([out[s] for s in range(n_slots)], 1), np.stack([lab[s] for s in range(n_slots)], 1)


def _check_interpolate(dev, model, setting, B, T, levels, max_batch, H, W, seed):
    frames, labels = _clip(B, T, H, W, seed)
    step = 1 << levels
    n_slots = (T - 1) * step + 1
    want_f, want_l = _reference_roll(model, dev, frames, labels, [t * step for t in range(T)], n_slots,
                                     midpoint_schedule(T, levels), max_batch, setting)
    f, l = _dev(dev, frames, labels)
    got_f, got_l = VideoSynthesizer(model, max_batch=max_batch, ensemble=setting).interpolate(f, l, levels=levels)
    assert got_f.shape == (B, n_slots, H, W, 3) and got_l.shape == (B, n_slots, H, W)
    got_f, got_l = got_f.cpu().numpy(), got_l.cpu().numpy()
    assert np.array_equal(got_f[:, ::step], frames) and np.array_equal(got_l[:, ::step], labels)  # originals
    assert np.array_equal(got_l, want_l)
    assert np.array_equal(got_f, want_f)
    # (and the ensemble did something: the plain synthesiser's frames differ)
    plain_f, _ = VideoSynthesizer(model, max_batch=max_batch).interpolate(f, l, levels=levels)
    assert not np.array_equal(plain_f.cpu().numpy(), got_f)


# (2, 3, 2, 2): per-triple chunks; (1, 4, 2, 3): gathered chunks that span triples
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("setting,B,T,levels,max_batch", [("time+flip", 2, 3, 2, 2), ("time", 1, 4, 2, 3)])
def test_interpolate_equals_composition(dev, precision, setting, B, T, levels, max_batch):
    model = _model(dev, "InterNet", precision=precision)
    _check_interpolate(dev, model, setting, B, T, levels, max_batch, 16, 32, 31)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_extrapolate_flip_equals_composition(dev, precision):
    B, H, W, steps = 3, 16, 32, 2
    model = _model(dev, "ExtraNet", "extra", precision)
    frames, labels = _clip(B, 2, H, W, 32)
    want_f, want_l = _reference_roll(model, dev, frames, labels, [0, 1], 2 + steps,
                                     [[(k, k + 1, k + 2)] for k in range(steps)], 2, "flip")
    got_f, got_l = VideoSynthesizer(model, max_batch=2, ensemble="flip").extrapolate(*_dev(dev, frames, labels), steps=steps)
    assert got_f.shape == (B, steps, H, W, 3) and got_l.shape == (B, steps, H, W)
    assert np.array_equal(got_l.cpu().numpy(), want_l[:, 2:])
    assert np.array_equal(got_f.cpu().numpy(), want_f[:, 2:])


def test_interpolate_stage3_equals_composition(dev):
    """every member a complete three-plan forward: a swap or a mirror that did not reach stage 3's
    neighbour frames and label maps, or bridges fed from the mean, would not pass"""
    model = _model(dev, "InterStage3Net", precision="bf16", prop=True)
    _check_interpolate(dev, model, "time+flip", B=1, T=3, levels=1, max_batch=3, H=64, W=128, seed=82)


# ---------------- the symmetries, through the public API ----------------
def test_flip_and_time_symmetries(dev):
    """With "flip" the mirrored clip gives the mirrored result, with "time" the reversed clip the same
    middle frame, frames and labels byte for byte: both sides run the same two forwards on the same
    batches, and a two-member fp32 sum is commutative.  Neither is asserted for "time+flip": there
    the transformed clip sums the same four members in another order ((x2 + x3) + x0) + x1 instead of
    ((x0 + x1) + x2) + x3, and fp32 addition is not associative.  The plain synthesiser on the same
    clips has neither symmetry (seed 1024, the other tests' default: no other seed was needed)."""
    B, H, W = 2, 16, 32
    model = _model(dev, "InterNet", precision="bf16", seed=1024)
    frames, labels = _clip(B, 2, H, W, 61)
    f, l = _dev(dev, frames, labels)
    fm, lm = _dev(dev, frames[:, :, :, ::-1], labels[:, :, :, ::-1])
    fr, lr = _dev(dev, frames[:, ::-1], labels[:, ::-1])

    def run(setting):
        syn = VideoSynthesizer(model, max_batch=2, ensemble=setting)
        return [tuple(t.cpu().numpy() for t in syn.interpolate(a, b, levels=1)) for a, b in ((f, l), (fm, lm), (fr, lr))]

    (pf, pl), (pfm, plm), _ = run("flip")
    assert np.array_equal(pfm, pf[:, :, :, ::-1]) and np.array_equal(plm, pl[:, :, :, ::-1])
    (pf, pl), _, (pfr, plr) = run("time")
    assert np.array_equal(pfr[:, 1], pf[:, 1]) and np.array_equal(plr[:, 1], pl[:, 1])
    assert np.array_equal(pfr, pf[:, ::-1]) and np.array_equal(plr, pl[:, ::-1])
    (pf, pl), (pfm, plm), (pfr, plr) = run(None)
    mirror = np.array_equal(pfm, pf[:, :, :, ::-1]) and np.array_equal(plm, pl[:, :, :, ::-1])
    reverse = np.array_equal(pfr[:, 1], pf[:, 1]) and np.array_equal(plr[:, 1], pl[:, 1])
    assert not (mirror and reverse)  # (the net is not symmetric by itself: the checks above are not vacuous)


# ---------------- on top of the other features ----------------
def _pad(a, Hp, Wp, hdim):
    iy, ix = np.minimum(np.arange(Hp), a.shape[hdim] - 1), np.minimum(np.arange(Wp), a.shape[hdim + 1] - 1)
    return np.take(np.take(a, iy, axis=hdim), ix, axis=hdim + 1)


def test_pad_replicate_equals_padding_by_hand(dev):
    """the mirror covers the whole canvas: the pad columns of a mirrored member are on the left"""
    B, H, W, levels = 2, 15, 30, 2
    model = _model(dev, "InterNet")
    frames, labels = _clip(B, 2, H, W, 71)
    syn = VideoSynthesizer(model, max_batch=2, pad="replicate", ensemble="time+flip")
    assert syn.canvas(H, W) == (16, 32)
    got_f, got_l = syn.interpolate(*_dev(dev, frames, labels), levels=levels)
    ref = VideoSynthesizer(model, max_batch=2, ensemble="time+flip")
    want_f, want_l = ref.interpolate(*_dev(dev, _pad(frames, 16, 32, 2), _pad(labels, 16, 32, 2)), levels=levels)
    assert got_f.shape == (B, 5, H, W, 3)
    assert torch.equal(got_f, want_f[:, :, :H, :W]) and torch.equal(got_l, want_l[:, :, :H, :W])


def test_tiles_equal_the_blend_of_per_tile_ensembles(dev):
    """the mirror is tile-local: an untiled ensemble synthesiser of the tile shape gives every
    tile's mean image and mean logits, tile_ref blends them"""
    B, H, W, tile, ov = 2, 24, 48, (16, 32), 8
    model = _model(dev, "InterNet", precision="bf16")
    frames, labels = _clip(B, 2, H, W, 72)
    f, l = _dev(dev, frames, labels)
    syn = VideoSynthesizer(model, max_batch=B, tile=tile, overlap=ov, ensemble="time+flip")
    assert len(syn.tiles(H, W)) == 4
    got_f, got_l = syn.interpolate(f, l, levels=1)
    ref = VideoSynthesizer(model, max_batch=B, ensemble="time+flip")
    ys, th = R.tile_starts(H, tile[0], ov, ref.multiple)
    xs, tw = R.tile_starts(W, tile[1], ov, ref.multiple)
    rgbs, segs = [], []
    for y0 in ys:
        for x0 in xs:
            crop = lambda t: t[:, y0:y0 + th, x0:x0 + tw].contiguous()  # noqa: E731
            xa, xb = (synth_load(crop(f[:, k]), torch.empty((B, th, tw, 8), dtype=torch.float32, device=dev)) for k in (0, 1))
            rgb = torch.empty((B, th, tw, 8), dtype=torch.float32, device=dev)
            ref._pair(xa, xb, crop(l[:, 0]), crop(l[:, 1]), rgb, torch.empty((B, th, tw, 3), dtype=torch.uint8, device=dev),
                      torch.empty((B, th, tw), dtype=torch.uint8, device=dev))
            rgbs.append(rgb.cpu().numpy())
            segs.append(ref._scratch_of(B, th, tw, dev)["seg"].cpu().numpy().copy())
    _, want_f, want_l, _ = R.blend(np.stack(rgbs), np.stack(segs), ys, xs, ov, H, W)
    assert np.array_equal(got_f[:, 1].cpu().numpy(), want_f) and np.array_equal(got_l[:, 1].cpu().numpy(), want_l)
    plain_f, _ = VideoSynthesizer(model, max_batch=B, tile=tile, overlap=ov).interpolate(f, l, levels=1)
    assert not torch.equal(plain_f[:, 1], got_f[:, 1])


def test_graph_replay_equals_eager(dev):
    B, H, W, levels = 2, 16, 32, 2
    model = _model(dev, "InterNet", precision="bf16")
    eager = VideoSynthesizer(model, max_batch=B, ensemble="time+flip")
    graphed = VideoSynthesizer(model, max_batch=B, graph=True, ensemble="time+flip")
    for seed in (41, 42):  # two different batches through the same captured graph
        f, l = _dev(dev, *_clip(B, 2, H, W, seed))
        ef, el = eager.interpolate(f, l, levels=levels)
        gf, gl = graphed.interpolate(f, l, levels=levels)
        torch.cuda.synchronize()
        assert torch.equal(ef, gf) and torch.equal(el, gl)
    assert len(graphed._graphs) == 1  # one graph holds the four members' forwards


def test_stream_equals_interpolate(dev):
    B, T, H, W, levels = 1, 3, 16, 32, 2
    model = _model(dev, "InterNet", precision="bf16")
    f, l = _dev(dev, *_clip(B, T, H, W, 73))
    syn = VideoSynthesizer(model, max_batch=1, ensemble="time")
    outs = list(syn.interpolate_stream(iter([(f[:, :2], l[:, :2]), (f[:, 2:], l[:, 2:])]), levels=levels))
    got_f, got_l = torch.cat([o[0] for o in outs], 1), torch.cat([o[1] for o in outs], 1)
    want_f, want_l = syn.interpolate(f, l, levels=levels)
    assert got_f.shape == (B, 9, H, W, 3) and torch.equal(got_f, want_f) and torch.equal(got_l, want_l)


def test_score_interpolation_scores_the_ensemble(dev):
    B, T, H, W = 2, 3, 16, 32
    model = _model(dev, "InterNet", precision="bf16")
    f, l = _dev(dev, *_clip(B, T, H, W, 74))
    syn = VideoSynthesizer(model, max_batch=2, ensemble="flip")
    sc = syn.score_interpolation(f, l, levels=1)
    want_f, want_l = syn.interpolate(f[:, ::2], l[:, ::2], levels=1)
    assert sc.slots == [1] and torch.equal(sc.frames, want_f) and torch.equal(sc.labels, want_l)
    assert sc.psnr.shape == (B, 1) and bool(torch.isfinite(sc.psnr).all())
    plain = VideoSynthesizer(model, max_batch=2).score_interpolation(f, l, levels=1)
    assert not torch.equal(plain.frames, sc.frames)


# ---------------- the launcher ----------------
def test_main_launcher_synth_ensemble(dev, tmp_path, caplog):
    """--split test --synth_ensemble flip over two PNG clips of three 16x32 frames: the PNGs decode to
    the API's arrays and the log names the ensemble; --synth_eval records it in scores.json, and
    without the flag the file has no such key"""
    from PIL import Image
    from deep_video_interpolation_extrapolation_amd import main as M
    H, W = 16, 32
    clips = {}
    data = tmp_path / "data"
    for seed, clip in enumerate(("aachen_000001", "bremen_000002")):
        clips[clip] = _clip(1, 3, H, W, 51 + seed, ignore=False)
        for sub, arr in zip(("rgb", "seg"), clips[clip]):
            (data / sub / clip).mkdir(parents=True)
            for t in range(3):
                Image.fromarray(arr[0, t]).save(data / sub / clip / f"{t:02d}.png")
    model = _model(dev, "InterNet", seed=7)
    run = tmp_path / "run"
    (run / "checkpoint").mkdir(parents=True)
    torch.save({"session": 0, "epoch": 2, "coarse_model": model.coarse_model.state_dict()},
               run / "checkpoint" / "InterNet_xs2xs_inter_0_1_0.pth")

    def launch(*flags):
        M.main(["--split", "test", "--syn_type", "inter", "--input_h", str(H), "--input_w", str(W), "--precision", "fp32",
                "--load_dir", str(run), "--checksession", "0", "--checkepoch", "1", "--checkpoint", "0",
                "--cycgen_load_dir", str(data)] + list(flags) + ["INTER", "--load_coarse"])

    with caplog.at_level(logging.INFO):
        launch("--synth_ensemble", "flip")
    assert "synth: self-ensemble flip: 2 forwards per predicted frame" in caplog.text
    syn = VideoSynthesizer(model, max_batch=1, ensemble="flip")
    for clip, (frames, labels) in clips.items():
        want_f, want_l = (t[0].cpu().numpy() for t in syn.interpolate(*_dev(dev, frames, labels), levels=1))
        for k in range(5):
            assert np.array_equal(np.asarray(Image.open(data / "synth" / "rgb" / clip / f"{k:04d}.png")), want_f[k])
            assert np.array_equal(np.asarray(Image.open(data / "synth" / "seg" / clip / f"{k:04d}.png")), want_l[k])
    plain_f = VideoSynthesizer(model, max_batch=1).interpolate(*_dev(dev, *clips["aachen_000001"]), levels=1)[0]
    assert not np.array_equal(plain_f[0].cpu().numpy(), np.stack(
        [np.asarray(Image.open(data / "synth" / "rgb" / "aachen_000001" / f"{k:04d}.png")) for k in range(5)]))

    launch("--synth_ensemble", "flip", "--synth_eval")
    got = json.loads((data / "synth_eval" / "scores.json").read_text())
    assert got["ensemble"] == "flip" and sorted(got["clips"]) == sorted(clips)
    for clip, (frames, labels) in clips.items():
        sc = syn.score_interpolation(*_dev(dev, frames, labels), levels=1)
        assert got["clips"][clip]["psnr"] == sc.psnr[0].cpu().numpy().tolist()
    caplog.clear()
    with caplog.at_level(logging.INFO):
        launch("--synth_eval")
    assert "self-ensemble" not in caplog.text
    assert "ensemble" not in json.loads((data / "synth_eval" / "scores.json").read_text())
    with pytest.raises(SystemExit):
        launch("--synth_ensemble", "vflip")


def test_main_launcher_extra_refuses_time(dev, tmp_path):
    """EXTRA with --synth_ensemble time ends the run with the constructor's error, before a clip is read"""
    from deep_video_interpolation_extrapolation_amd import main as M
    model = _model(dev, "ExtraNet", "extra", seed=7)
    run, data = tmp_path / "run", tmp_path / "data"
    (run / "checkpoint").mkdir(parents=True)
    (data / "rgb").mkdir(parents=True)
    torch.save({"session": 0, "epoch": 2, "coarse_model": model.coarse_model.state_dict()},
               run / "checkpoint" / "ExtraNet_xs2xs_extra_0_1_0.pth")
    for setting in ("time", "time+flip"):
        with pytest.raises(ValueError, match="extrapolation has no time symmetry"):
            M.main(["--split", "test", "--syn_type", "extra", "--input_h", "16", "--input_w", "32", "--precision", "fp32",
                    "--load_dir", str(run), "--checksession", "0", "--checkepoch", "1", "--checkpoint", "0",
                    "--cycgen_load_dir", str(data), "--synth_ensemble", setting, "EXTRA", "--load_coarse",
                    "--num_pred_step", "2"])
