"""GPU checks of tiled synthesis (VideoSynthesizer(tile=, overlap=), synth.tile_blend).

* dvie_synth_tile_blend against the numpy restatement tests/tile_ref.py, bit for bit: the fp32
  canvas, the frame, the label and the label canvas, with guard bytes around every output;
* the synthesiser end to end: the expected frames are built in the test tile by tile -- an untiled
  synthesiser of the tile shape gives every tile's raw image and coarse logits, tile_ref blends them
  -- and must match byte for byte; the untiled path when the canvas fits a tile; pad, the two-stage
  net, graph replay, streaming and the `--split test --synth_tile` command.

Every comparison is array_equal.  The inputs are finite (the blend of a NaN is not specified)."""
import types

import numpy as np
import pytest
import torch

import tile_ref as R
from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import nets
from deep_video_interpolation_extrapolation_amd.synth import VideoSynthesizer, synth_load, tile_blend

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 77
TILE, OV = (24, 40), 8


# ---------------- the kernel ----------------
def _tile_inputs(nt, n, th, tw, ys, xs, seed):
    """independent finite tile values (nothing is cut from one map: the blend has work to do); rgb
    with finish's half-points and values outside [-1, 1], padding channels NaN; logits with tie
    rows at single-covered and at seam pixels, padding channels +inf"""
    rng = np.random.RandomState(seed)
    rgb = np.full((nt, n, th, tw, 8), np.nan, dtype=F32)
    vals = rng.uniform(-1.3, 1.3, (nt, n, th, tw, 3)).astype(F32)
    half = (((np.arange(255, dtype=np.float64) + 0.5) / 127.5) - 1.0).astype(F32)
    flat = vals.reshape(-1)
    flat[rng.permutation(flat.size)[:4 * half.size]] = np.tile(half, 4)
    rgb[..., :3] = vals
    seg = np.full((nt, n, th, tw, 24), np.inf, dtype=F32)
    seg[..., :20] = rng.randn(nt, n, th, tw, 20).astype(F32)
    # ties: at some canvas pixels every covering tile gets the same top value in several classes
    hp, wp = ys[-1] + th, xs[-1] + tw
    rows = [([0, 19], 9.0), ([3, 7], 8.0), ([0, 5, 19], 7.5), ([4, 11, 12], 7.0), ([18, 19], 6.0), (list(range(20)), 0.25)]
    pts = [(rng.randint(hp), rng.randint(wp)) for _ in range(40)] + [(hp - 1, wp - 1), (0, 0), (ys[-1], xs[-1]),
                                                                     (ys[-1] + 1, xs[-1] + 2)]
    for k, (y, x) in enumerate(pts):
        cls, v = rows[k % len(rows)]
        t = 0
        for y0 in ys:
            for x0 in xs:
                if y0 <= y < y0 + th and x0 <= x < x0 + tw:
                    seg[t, :, y - y0, x - x0, cls] = v
                t += 1
    return rgb, seg


def _guarded(dev, shape, lead=1, dtype=torch.uint8, fill=GUARD):
    """a tensor of `shape`, `lead` elements into its allocation, guard elements around it"""
    size = int(np.prod(shape))
    buf = torch.full((size + 2 * lead,), fill, dtype=dtype, device=dev)
    return buf, buf[lead:lead + size].view(shape)


def _guards_intact(buf, lead=1, fill=GUARD):
    return bool((buf[:lead] == fill).all()) and bool((buf[-lead:] == fill).all())


# canvas, tile, overlap, (h, w), n
CASES = {
    "44x72_crop41x70_n2": ((44, 72), (24, 40), 8, (41, 70), 2),  # rows 20..23 under three tiles, columns 32..39 under two
    "24x88_rows_untiled": ((24, 88), (24, 40), 8, (24, 88), 1),
    "44x72_overlap0": ((44, 72), (24, 40), 0, (44, 72), 1),
    "48x72_m8_crop": ((48, 72), (24, 40), 8, (45, 65), 1),
}


@pytest.mark.parametrize("case", list(CASES))
def test_tile_blend_kernel_bit_exact(dev, case):
    (hp, wp), (th, tw), ov, (h, w), n = CASES[case]
    m = 8 if "m8" in case else 4
    ys, eh = R.tile_starts(hp, th, ov, m)
    xs, ew = R.tile_starts(wp, tw, ov, m)
    nt = len(ys) * len(xs)
    cover = (R.weights(ys, xs, eh, ew, ov) > 0).sum(0)
    if case.startswith("44x72_crop"):
        assert ys == [0, 8, 20] and (cover[20:24] >= 3).all() and cover.max() == 6 and (cover == 1).any()
    if case.startswith("24x88"):
        assert ys == [0] and eh == 24 and len(xs) == 3
    rgb, seg = _tile_inputs(nt, n, eh, ew, ys, xs, seed=len(case))
    want_rgb, want_frame, want_label, want_canvas = R.blend(rgb, seg, ys, xs, ov, h, w)
    rgb_t, seg_t = torch.from_numpy(rgb).to(dev), torch.from_numpy(seg).to(dev)
    # every output; rgb_out NULL; label_canvas NULL, and 1 byte into its allocation (bytewise stores)
    for with_rgb, canvas_lead in ((True, 4), (False, 4), (True, None), (True, 1)):
        fbuf, frame = _guarded(dev, (n, h, w, 3))
        lbuf, label = _guarded(dev, (n, h, w))
        rbuf, rgb_out = _guarded(dev, (n, hp, wp, 8), 4, torch.float32, 123.0) if with_rgb else (None, None)
        cbuf, lcan = _guarded(dev, (n, hp, wp), canvas_lead) if canvas_lead else (None, None)
        tile_blend(rgb_t, seg_t, ys, xs, ov, frame, label, rgb_out, lcan)
        assert np.array_equal(frame.cpu().numpy(), want_frame)
        assert np.array_equal(label.cpu().numpy(), want_label)
        assert _guards_intact(fbuf) and _guards_intact(lbuf)
        if with_rgb:
            got = rgb_out.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want_rgb.view(np.uint32))
            assert not got[..., 3:].view(np.uint32).any()  # channels 3 and up: zero bits
            assert _guards_intact(rbuf, 4, 123.0)
        if canvas_lead:
            assert np.array_equal(lcan.cpu().numpy(), want_canvas)
            assert _guards_intact(cbuf, canvas_lead)
    # the ties were decided for the lowest index, also on seams
    top = np.sort(R.blend_map(seg[..., :20], ys, xs, ov), axis=-1)
    tied = top[..., -1] == top[..., -2]
    assert tied[:, cover > 1].any() and tied[:, cover == 1].any()


# ---------------- the synthesiser ----------------
def _args(kind="inter", precision="fp32", large=False, n_scales=2, prop=False):
    return types.SimpleNamespace(syn_type=kind, highres_large=large, coarse_model="HRNet", precision=precision,
                                 n_scales=n_scales, stage3_prop=prop, refine_model="SRNRefine",
                                 stage3_model="MSResAttnRefine")


def _model(dev, name, seed=1024, **kw):
    torch.manual_seed(seed)
    return nets.__dict__[name](_args(**kw)).to(dev).eval()


def _clip(dev, B, T, H, W, seed):
    rng = np.random.RandomState(seed)
    frames = rng.randint(0, 256, (B, T, H, W, 3)).astype(np.uint8)
    labels = rng.randint(0, 20, (B, T, H, W)).astype(np.uint8)
    labels[rng.rand(B, T, H, W) < 0.05] = 255  # Cityscapes' "ignore"
    return torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)


def _expected_pair(model, fa, fb, la, lb, tile=TILE, overlap=OV):
    """the tiled prediction from uint8 frames fa, fb (n, H, W, 3) and labels (n, H, W), H and W
    multiples of the net's stride, built tile by tile: an untiled synthesiser of the tile shape runs
    each crop (its _pair writes the raw rgb and leaves the coarse logits in its scratch), and tile_ref
    blends what it gave -> (frame, label, label canvas) as numpy arrays"""
    dev = fa.device
    ref = VideoSynthesizer(model, max_batch=fa.shape[0])
    n, H, W, _ = fa.shape
    m = ref.multiple
    ys, th = R.tile_starts(H, tile[0], overlap, m)
    xs, tw = R.tile_starts(W, tile[1], overlap, m)
    rgbs, segs = [], []
    for y0 in ys:
        for x0 in xs:
            crop = lambda t: t[:, y0:y0 + th, x0:x0 + tw].contiguous()  # noqa: E731
            xa = synth_load(crop(fa), torch.empty((n, th, tw, 8), dtype=torch.float32, device=dev))
            xb = synth_load(crop(fb), torch.empty((n, th, tw, 8), dtype=torch.float32, device=dev))
            rgb = torch.empty((n, th, tw, 8), dtype=torch.float32, device=dev)
            frame = torch.empty((n, th, tw, 3), dtype=torch.uint8, device=dev)
            label = torch.empty((n, th, tw), dtype=torch.uint8, device=dev)
            ref._pair(xa, xb, crop(la), crop(lb), rgb, frame, label)
            rgbs.append(rgb.cpu().numpy())
            segs.append(ref._scratch_of(n, th, tw, dev)["seg"].cpu().numpy().copy())
    rgbs, segs = np.stack(rgbs), np.stack(segs)
    assert np.isfinite(rgbs[..., :3]).all() and np.isfinite(segs[..., :20]).all()
    _, frame, label, canvas = R.blend(rgbs, segs, ys, xs, overlap, H, W)
    return frame, label, canvas


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_interpolate_coarse_equals_the_per_tile_construction(dev, precision):
    B, H, W = 2, 44, 72
    model = _model(dev, "InterNet", precision=precision)
    f, l = _clip(dev, B, 2, H, W, 71)
    syn = VideoSynthesizer(model, max_batch=B, tile=TILE, overlap=OV)
    assert len(syn.tiles(H, W)) == 6
    got_f, got_l = syn.interpolate(f, l, levels=1)
    assert got_f.shape == (B, 3, H, W, 3) and got_l.shape == (B, 3, H, W)
    assert torch.equal(got_f[:, ::2], f) and torch.equal(got_l[:, ::2], l)  # the input slots, bit for bit
    want_f, want_l, _ = _expected_pair(model, f[:, 0], f[:, 1], l[:, 0], l[:, 1])
    assert np.array_equal(got_l[:, 1].cpu().numpy(), want_l)
    assert np.array_equal(got_f[:, 1].cpu().numpy(), want_f)
    # (and tiling did something: the untiled frame differs)
    plain_f, _ = VideoSynthesizer(model, max_batch=B).interpolate(f, l, levels=1)
    assert not torch.equal(plain_f[:, 1], got_f[:, 1])


def test_levels_and_extrapolation_are_deterministic(dev):
    B, H, W = 2, 44, 72
    model = _model(dev, "InterNet", precision="bf16")
    f, l = _clip(dev, B, 3, H, W, 72)
    f0, l0 = f.clone(), l.clone()
    syn = VideoSynthesizer(model, max_batch=2, tile=TILE, overlap=OV)
    a_f, a_l = syn.interpolate(f, l, levels=2)
    b_f, b_l = syn.interpolate(f, l, levels=2)
    assert a_f.shape == (B, 9, H, W, 3) and a_l.shape == (B, 9, H, W)
    assert torch.equal(a_f, b_f) and torch.equal(a_l, b_l)
    assert torch.equal(a_f[:, ::4], f0) and torch.equal(a_l[:, ::4], l0) and torch.equal(f, f0) and torch.equal(l, l0)
    # B = 1, max_batch = 3: the gather path, level 1's two triples in one tiled forward of two pairs
    one = VideoSynthesizer(model, max_batch=3, tile=TILE, overlap=OV)
    c_f, c_l = one.interpolate(f[:1], l[:1], levels=2)
    d_f, d_l = one.interpolate(f[:1], l[:1], levels=2)
    assert c_f.shape == (1, 9, H, W, 3) and torch.equal(c_f, d_f) and torch.equal(c_l, d_l)
    want_f, want_l, _ = _expected_pair(model, f[0, :2], f[0, 1:], l[0, :2], l[0, 1:])
    assert np.array_equal(c_f[0, 2:7:4].cpu().numpy(), want_f) and np.array_equal(c_l[0, 2:7:4].cpu().numpy(), want_l)
    ext = _model(dev, "ExtraNet", kind="extra", precision="fp32")
    syn = VideoSynthesizer(ext, max_batch=2, tile=TILE, overlap=OV)
    e_f, e_l = syn.extrapolate(f[:, :2], l[:, :2], steps=2)
    g_f, g_l = syn.extrapolate(f[:, :2], l[:, :2], steps=2)
    assert e_f.shape == (B, 2, H, W, 3) and e_l.shape == (B, 2, H, W)
    assert torch.equal(e_f, g_f) and torch.equal(e_l, g_l) and torch.equal(f, f0) and torch.equal(l, l0)
    # step 1 is the per-tile construction; step 2 read step 1's kept fp32 form (not its uint8 frame)
    want_f, want_l, _ = _expected_pair(ext, f[:, 0], f[:, 1], l[:, 0], l[:, 1])
    assert np.array_equal(e_f[:, 0].cpu().numpy(), want_f) and np.array_equal(e_l[:, 0].cpu().numpy(), want_l)
    assert not torch.equal(e_f[:, 0], e_f[:, 1])


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


@pytest.mark.parametrize("tile", [(44, 72), (48, 80)])
def test_a_canvas_that_fits_one_tile_takes_the_untiled_path(dev, tile):
    H, W = 44, 72
    model = _model(dev, "InterNet", precision="bf16")
    f, l = _clip(dev, 2, 3, H, W, 73)
    plain, tiled = VideoSynthesizer(model, max_batch=2), VideoSynthesizer(model, max_batch=2, tile=tile, overlap=OV)
    assert tiled.tiles(H, W) == [(0, 0, H, W)]
    (want_f, want_l), want_names = _traced(lambda: plain.interpolate(f, l, levels=2))
    (got_f, got_l), got_names = _traced(lambda: tiled.interpolate(f, l, levels=2))
    assert torch.equal(got_f, want_f) and torch.equal(got_l, want_l)
    assert got_names == want_names and "synth_finish_kernel" in got_names and "tile_blend" not in got_names
    assert not tiled._tile_scratch  # nothing was allocated for tiling
    # and a tiled run does launch it
    _, names = _traced(lambda: VideoSynthesizer(model, max_batch=2, tile=TILE, overlap=OV).interpolate(f[:, :2], l[:, :2], levels=1))
    assert names.count("synth_tile_blend_kernel") == 1 and "synth_finish_kernel" not in names


def test_an_oversized_forward_is_refused_before_anything_is_launched(dev):
    """the guard of the public entry points, with the limit set low (the real one needs a UHD frame)"""
    from deep_video_interpolation_extrapolation_amd.synth import FrameSizeError
    H, W = 44, 72
    model = _model(dev, "InterNet", precision="bf16")
    f, l = _clip(dev, 1, 3, H, W, 80)
    for kw, what in ((dict(), "the 44x72 canvas"), (dict(tile=(32, 72), overlap=OV), "a tile of 32x72")):
        syn = VideoSynthesizer(model, max_batch=1, **kw)
        assert syn.max_pixels == 4793489
        syn._max_pixels = 24 * 72  # (a 24x72 forward would still fit)
        for call in (lambda: syn.interpolate(f, l, levels=1), lambda: syn.extrapolate(f[:, :2], l[:, :2], steps=1),
                     lambda: list(syn.interpolate_stream(iter([(f, l)]), levels=1)), lambda: syn.score_extrapolation(f, l)):
            lib = L.load()
            lib.dvie_trace_kernels(1)
            try:
                with pytest.raises(FrameSizeError, match=what + ".*tile=") as e:
                    call()
                torch.cuda.synchronize()
                assert e.value.too_large and lib.dvie_traced_kernels().decode() == ""  # nothing was launched
            finally:
                lib.dvie_trace_kernels(0)
    ok = VideoSynthesizer(model, max_batch=1, tile=(24, 72), overlap=OV)
    ok._max_pixels = 24 * 72
    assert ok.interpolate(f, l, levels=1)[0].shape == (1, 5, H, W, 3)


def _pad_t(t, Hp, Wp, hdim):
    H, W = t.shape[hdim], t.shape[hdim + 1]
    iy = torch.arange(Hp, device=t.device).clamp(max=H - 1)
    ix = torch.arange(Wp, device=t.device).clamp(max=W - 1)
    return t.index_select(hdim, iy).index_select(hdim + 1, ix).contiguous()


def test_pad_replicate_with_tiles_equals_padding_by_hand(dev):
    B, H, W, levels = 2, 41, 70, 2
    model = _model(dev, "InterNet", precision="fp32")
    f, l = _clip(dev, B, 2, H, W, 74)
    syn = VideoSynthesizer(model, max_batch=2, pad="replicate", tile=TILE, overlap=OV)
    assert syn.canvas(H, W) == (44, 72) and len(syn.tiles(H, W)) == 6
    got_f, got_l = syn.interpolate(f, l, levels=levels)
    assert got_f.shape == (B, 5, H, W, 3) and got_f.stride()[2:] == (W * 3, 3, 1)
    ref = VideoSynthesizer(model, max_batch=2, tile=TILE, overlap=OV)
    want_f, want_l = ref.interpolate(_pad_t(f, 44, 72, 2), _pad_t(l, 44, 72, 2), levels=levels)
    assert torch.equal(got_f, want_f[:, :, :H, :W]) and torch.equal(got_l, want_l[:, :, :H, :W])
    assert torch.equal(got_f[:, ::4], f) and torch.equal(got_l[:, ::4], l)


def test_stage3_net_equals_the_per_tile_construction(dev):
    B, H, W = 1, 48, 72
    model = _model(dev, "InterStage3Net", precision="bf16", n_scales=2)
    f, l = _clip(dev, B, 2, H, W, 75)
    syn = VideoSynthesizer(model, max_batch=1, tile=TILE, overlap=OV)
    assert syn.multiple == 8 and [t[:2] for t in syn.tiles(H, W)] == [(y, x) for y in (0, 8, 24) for x in (0, 32)]
    got_f, got_l = syn.interpolate(f, l, levels=1)
    want_f, want_l, _ = _expected_pair(model, f[:, 0], f[:, 1], l[:, 0], l[:, 1])
    assert np.array_equal(got_f[:, 1].cpu().numpy(), want_f) and np.array_equal(got_l[:, 1].cpu().numpy(), want_l)
    assert torch.equal(got_f[:, ::2], f) and torch.equal(got_l[:, ::2], l)


def test_graph_replay_equals_eager(dev):
    B, H, W, steps = 2, 41, 70, 2
    model = _model(dev, "ExtraNet", kind="extra", precision="bf16")
    eager = VideoSynthesizer(model, max_batch=B, pad="replicate", tile=TILE, overlap=OV)
    graphed = VideoSynthesizer(model, max_batch=B, graph=True, pad="replicate", tile=TILE, overlap=OV)
    for seed in (76, 77):  # two different batches through the same captured graph
        f, l = _clip(dev, B, 2, H, W, seed)
        ef, el = eager.extrapolate(f, l, steps=steps)
        gf, gl = graphed.extrapolate(f, l, steps=steps)
        torch.cuda.synchronize()
        assert gf.shape == (B, steps, H, W, 3) and torch.equal(ef, gf) and torch.equal(el, gl)
    assert len(graphed._graphs) == 1 and next(iter(graphed._graphs))[:3] == (B,) + TILE  # one graph: the tile's
    graphed.reset()
    assert not graphed._tile_scratch


def test_stream_equals_interpolate_per_window(dev):
    B, T, H, W, levels = 1, 5, 44, 72, 1
    model = _model(dev, "InterNet", precision="bf16")
    f, l = _clip(dev, B, T, H, W, 78)
    syn = VideoSynthesizer(model, max_batch=2, tile=TILE, overlap=OV)
    outs = list(syn.interpolate_stream(iter([(f[:, :3], l[:, :3]), (f[:, 3:], l[:, 3:])]), levels=levels))
    got_f, got_l = torch.cat([o[0] for o in outs], 1), torch.cat([o[1] for o in outs], 1)
    parts = [syn.interpolate(f[:, a:b + 1], l[:, a:b + 1], levels) for a, b in ((0, 2), (2, 4))]
    want_f = torch.cat([parts[0][0], parts[1][0][:, 1:]], 1)
    want_l = torch.cat([parts[0][1], parts[1][1][:, 1:]], 1)
    assert got_f.shape == (B, 9, H, W, 3) and torch.equal(got_f, want_f) and torch.equal(got_l, want_l)


# ---------------- the launcher ----------------
@pytest.mark.parametrize("runner,kind,name", [("INTER", "inter", "InterNet"), ("EXTRA", "extra", "ExtraNet")])
def test_main_launcher_synth_tile(dev, tmp_path, runner, kind, name):
    """--split test --synth_tile 24x40 --synth_tile_overlap 8 over a 44x72 clip of three PNG frames:
    the files written are the Python API's arrays, and the blend kernel ran"""
    from PIL import Image
    from deep_video_interpolation_extrapolation_amd import main as M
    H, W, clip = 44, 72, "aachen_000001"
    data = tmp_path / "data"
    f, l = _clip(dev, 1, 3, H, W, 79)
    l = l.clamp(max=19)
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

    with pytest.raises(ValueError, match="multiple 4"):
        launch("--synth_tile", "22x40", "--synth_tile_overlap", "8")
    _, names = _traced(lambda: launch("--synth_tile", "24x40", "--synth_tile_overlap", "8"))
    assert "synth_tile_blend_kernel" in names
    syn = VideoSynthesizer(model, max_batch=1, tile=TILE, overlap=OV)
    want_f, want_l = syn.interpolate(f, l, levels=1) if runner == "INTER" else syn.extrapolate(f[:, -2:], l[:, -2:], 2)
    want_f, want_l = want_f[0].cpu().numpy(), want_l[0].cpu().numpy()
    assert want_f.shape == (n_out, H, W, 3)
    for sub in ("rgb", "seg", "vis_seg"):
        files = sorted(p.name for p in (data / "synth" / sub / clip).iterdir())
        assert files == [f"{k:04d}.png" for k in range(n_out)], (runner, sub, files)
    for k in range(n_out):
        assert np.array_equal(np.asarray(Image.open(data / "synth" / "rgb" / clip / f"{k:04d}.png")), want_f[k])
        assert np.array_equal(np.asarray(Image.open(data / "synth" / "seg" / clip / f"{k:04d}.png")), want_l[k])
