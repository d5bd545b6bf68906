"""GPU checks of the per-frame VGG19 perceptual score (synth.PerceptualScorer): the load kernel
bit for bit, the per-image cosine reduction against numpy float64, the score against the float64
oracle one frame at a time, chunking, determinism, the arena against one buffer per activation,
and the plumbing through frame_scores, score_interpolation / score_extrapolation and the
`--split test --synth_eval --synth_vgg` launcher.

Measured worst deviations (MI355X; DESIGN.md "Perceptual score (--synth_vgg)" has the table):
cosine op against numpy float64 1.2e-7 (gate 1e-4); per-frame score against the float64 oracle
over 16x16, 32x64 and 37x53 and the four kinds of `pred`: fp32 5.5e-8 (gate 1e-5), bf16 2.4e-4
(gate 2e-2); chunkings agree to the bit.  Every test prints its figures (run with -s)."""
import ctypes
import functools
import json
import types

import numpy as np
import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import nets, synth
from deep_video_interpolation_extrapolation_amd.synth import PerceptualScorer, VideoSynthesizer, frame_scores
from oracle import losses as OL

pytestmark = pytest.mark.gpu
DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16}
GATE = {"fp32": 1e-5, "bf16": 2e-2}  # the project's VGG-cosine gates (test_gpu_metrics.py)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _bits(t):
    return t.contiguous().cpu().view(torch.int16 if t.element_size() == 2 else (torch.int32 if t.element_size() == 4
                                                                                  else torch.int64)).numpy()


_SCORERS = {}


def _scorer(monkeypatch, prec, max_batch):
    """one scorer per (precision, max_batch) for the module: the synthetic weights and the plans
    are built once"""
    monkeypatch.setenv("DVIE_PRECISION", prec)
    if (prec, max_batch) not in _SCORERS:
        _SCORERS[prec, max_batch] = PerceptualScorer(max_batch=max_batch)
        assert _SCORERS[prec, max_batch].net.dtype == DTYPE[prec]
    return _SCORERS[prec, max_batch]


# ---------------- 1. load kernel ----------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_load_kernel_bit_exact(dev, prec):
    dtype, H, W, h16, w16, B, S = DTYPE[prec], 37, 53, 32, 48, 2, 3
    assert synth.vgg_region(H, W) == (h16, w16)
    rng = np.random.RandomState(5)
    nbytes = S * B * H * W * 3
    raw = [torch.from_numpy(rng.randint(0, 256, nbytes + 1).astype(np.uint8)).to(dev) for _ in range(2)]
    store = [r[1:].view(S, B, H, W, 3) for r in raw]  # slot-major, 1 byte into the allocation
    pred, gt = store[0].transpose(0, 1), store[1].transpose(0, 1)  # (B, S) strided views
    assert pred.data_ptr() % 2 == 1 and gt.data_ptr() % 2 == 1 and not pred.is_contiguous()
    lut = synth.vgg_lut(dtype)
    lut_bits = _bits(lut)
    lut_dev = lut.to(dev)

    def run():
        out = torch.empty((2 * B * S, h16, w16, 8), dtype=dtype, device=dev)
        out.view(torch.int16 if prec == "bf16" else torch.int32).fill_(0x7FC0 if prec == "bf16" else 0x7FC00000)
        assert bool(torch.isnan(out).all())
        synth.vgg_load(pred, gt, out, lut_dev)
        return _bits(out)

    def want():
        imgs = np.concatenate([t.cpu().numpy().reshape(B * S, H, W, 3) for t in (pred, gt)])[:, :h16, :w16]
        exp = np.zeros((2 * B * S, h16, w16, 8), dtype=lut_bits.dtype)
        for c in range(3):
            exp[..., c] = lut_bits[c][imgs[..., c]]
        return exp

    got, exp = run(), want()
    assert got.shape == exp.shape and np.array_equal(got[..., :3], exp[..., :3])
    assert not got[..., 3:].any()  # channels 3..7: zero bits, not the NaN fill
    # [pred | gt]: image i0 * S + i1 of each half is frame (i0, i1)
    assert np.array_equal(got[1 * S + 2, ..., 0], lut_bits[0][pred[1, 2, :h16, :w16, 0].cpu().numpy()])
    assert np.array_equal(got[B * S + 0 * S + 1, ..., 2], lut_bits[2][gt[0, 1, :h16, :w16, 2].cpu().numpy()])
    # rows 32..36 and columns 48..52 are not read
    for s in store:
        s[:, :, h16:] ^= 0xFF
        s[:, :, :, w16:] ^= 0xFF
    assert np.array_equal(run(), got) and np.array_equal(want(), exp)


# ---------------- 2. cosine op ----------------
def _cosfeat(feat, n, c):
    """dvie_cosfeat over one tap: feat (2n, h, w, ld) -> n float64"""
    lib = L.load()
    _, h, w, ld = feat.shape
    d = L.CosFeatDesc()
    d.feat, d.ld, d.dtype = feat.data_ptr(), ld, L.BF16 if feat.dtype == torch.bfloat16 else L.F32
    d.n, d.h, d.w, d.c, d.tap, d.n_taps = n, h, w, c, 0, 1
    blocks = lib.dvie_cosfeat_blocks(ctypes.byref(d))
    assert blocks >= 1
    ws = torch.full((n * blocks,), float("nan"), dtype=torch.float64, device=feat.device)
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=feat.device)
    d.ws, d.out, d.ws_blocks = ws.data_ptr(), out.data_ptr(), blocks
    d.blocks[0], d.px[0] = blocks, h * w
    L.check(lib.dvie_cosfeat(ctypes.byref(d), L.stream_ptr(feat.device)), "cosfeat")
    d.mode = 1
    L.check(lib.dvie_cosfeat(ctypes.byref(d), L.stream_ptr(feat.device)), "cosfeat finalize")
    return out.cpu().numpy()


def _cos_ref(feat, n, c):
    f = feat[..., :c].double().cpu().numpy()
    a, b = f[:n], f[n:]
    cos = (a * b).sum(-1) / (np.sqrt((a * a).sum(-1)) * np.sqrt((b * b).sum(-1)))
    return cos.reshape(n, -1).mean(1)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("c", [64, 128, 256, 512])
def test_cosine_op_against_numpy_float64(dev, prec, c):
    n, worst = 3, 0.0
    g = torch.Generator().manual_seed(100 + c)
    for h, w in ((5, 7), (1, 1), (40, 52)):  # (40 x 52: more than one block per image at every c)
        for ld in (c, c + 16):
            feat = torch.rand((2 * n, h, w, ld), generator=g).to(DTYPE[prec]).to(dev)
            got, ref = _cosfeat(feat, n, c), _cos_ref(feat, n, c)
            worst = max(worst, float(np.abs(got - ref).max()))
            print(f"cosfeat {prec} c={c} {h}x{w} ld={ld}: max |dev - float64| = {np.abs(got - ref).max():.3e}")
            assert np.isfinite(got).all() and np.abs(got - ref).max() <= 1e-4, (h, w, ld, got, ref)
    print(f"cosfeat {prec} c={c}: worst {worst:.3e}")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_cosine_op_identical_halves_and_zero_pixel(dev, prec):
    n, c, h, w = 3, 128, 5, 7
    g = torch.Generator().manual_seed(7)
    half = torch.rand((n, h, w, c), generator=g).to(DTYPE[prec])
    same = _cosfeat(torch.cat([half, half]).to(dev), n, c)
    print(f"cosfeat {prec} identical halves: 1 - value = {1 - same}")
    assert (1 - same <= 1e-6).all() and (same - 1 <= 1e-6).all()
    feat = torch.rand((2 * n, h, w, c), generator=g).to(DTYPE[prec])
    base = _cosfeat(feat.to(dev), n, c)
    feat[1, 2, 3] = 0  # one all-zero pixel of image 1, prediction side
    got = _cosfeat(feat.to(dev), n, c)
    assert np.isnan(got[1]) and np.isfinite(base).all()
    assert got[[0, 2]].tobytes() == base[[0, 2]].tobytes()


# ---------------- 3. the score against the oracle ----------------
KINDS = ("random", "noise", "equal", "zero")


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """five pairs per kind of `pred` and their float64 oracle values, computed once per size"""
    rng = np.random.RandomState(H * 1000 + W)
    gt = rng.randint(0, 256, (5, H, W, 3)).astype(np.uint8)
    pred = dict(random=rng.randint(0, 256, gt.shape).astype(np.uint8),
                noise=np.clip(gt.astype(np.int16) + rng.randint(-6, 7, gt.shape), 0, 255).astype(np.uint8),
                equal=gt.copy(), zero=np.zeros_like(gt))
    state = {k: v.double() for k, v in OL.synthetic_vgg19_state().items()}
    h16, w16 = synth.vgg_region(H, W)

    def f64(x):  # uint8 (H, W, 3) -> float64 NCHW [0, 1] of the scored region
        return torch.from_numpy(x[:h16, :w16]).permute(2, 0, 1)[None].double() / 255

    with torch.no_grad():
        ref = {k: np.array([float(OL.vgg_cosine(state, f64(p[i]), f64(gt[i]), normed=False)) for i in range(5)])
               for k, p in pred.items()}
    return gt, pred, ref


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("H,W", [(16, 16), (32, 64), (37, 53)])
def test_score_against_float64_oracle(dev, monkeypatch, prec, H, W):
    gt, pred, ref = _case(H, W)
    s = _scorer(monkeypatch, prec, 2)  # chunks of 2, 2 and 1
    g = torch.from_numpy(gt).to(dev)
    got = {}
    for k in KINDS:
        v = s(torch.from_numpy(pred[k]).to(dev), g)
        assert v.dtype == torch.float64 and tuple(v.shape) == (5,) and v.device == g.device
        got[k] = v.cpu().numpy()
        print(f"vgg {prec} {H}x{W} {k}: oracle {ref[k]} device {got[k]} max |diff| {np.abs(got[k] - ref[k]).max():.3e}")
    for k in KINDS:
        assert np.isfinite(ref[k]).all() and np.isfinite(got[k]).all(), k
        assert np.abs(got[k] - ref[k]).max() <= GATE[prec], (k, got[k], ref[k])
    assert (got["equal"] >= 1 - 1e-6).all() and (1 - 1e-6 > got["noise"]).all() and (got["noise"] > got["random"]).all()


# ---------------- 4. chunking ----------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_chunking(dev, monkeypatch, prec):
    gt, pred, ref = _case(32, 64)
    mix = ("random", "noise", "equal", "zero", "random")  # distinct frames with far-apart scores
    p = torch.from_numpy(np.stack([pred[k][i] for i, k in enumerate(mix)])).to(dev)
    want = np.array([ref[k][i] for i, k in enumerate(mix)])
    g = torch.from_numpy(gt).to(dev)
    by2 = _scorer(monkeypatch, prec, 2)(p, g).cpu().numpy()
    s8 = _scorer(monkeypatch, prec, 8)
    by8 = s8(p, g).cpu().numpy()
    single = np.array([float(s8(p[i], g[i])) for i in range(5)])
    assert s8(p[0], g[0]).shape == () and s8(p[None], g[None]).shape == (1, 5)
    print(f"chunking {prec}: 2 vs 8 {np.abs(by2 - by8).max():.3e}, 1 vs 8 {np.abs(single - by8).max():.3e}")
    assert np.abs(by2 - by8).max() <= GATE[prec] and np.abs(single - by8).max() <= GATE[prec]
    # a mis-indexed frame differs by far more than the gate: each value is its own frame's
    for v in (by2, by8, single):
        assert np.abs(v - want).max() <= GATE[prec], (v, want)


# ---------------- 5. determinism and arena ----------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_determinism_and_arena(dev, monkeypatch, prec):
    gt, pred, _ = _case(32, 64)
    p, g = torch.from_numpy(pred["noise"]).to(dev), torch.from_numpy(gt).to(dev)
    s = _scorer(monkeypatch, prec, 8)
    a, b = s(p, g), s(p, g)
    assert _bits(a).tobytes() == _bits(b).tobytes()
    arena = s.net.score_plan(5, 32, 64, dev)
    plain = s.net.score_plan(5, 32, 64, dev, alias=False)
    assert arena.alias and not plain.alias and arena.arena_bytes < plain.unaliased_bytes
    synth.vgg_load(p, g, plain.input_view("vgg_in"), synth.vgg_lut(DTYPE[prec]).to(dev))
    ws = torch.empty((plain.cosfeat_ws_doubles,), dtype=torch.float64, device=dev)
    out = torch.empty((5,), dtype=torch.float64, device=dev)
    plain.set_cosfeat(ws, out)
    plain.run_forward()
    assert _bits(out).tobytes() == _bits(a).tobytes()


# ---------------- 6. plumbing ----------------
NC = 20


def _net(kind="inter", seed=1024):
    a = types.SimpleNamespace(syn_type=kind, highres_large=False, coarse_model="HRNet", precision="fp32")
    torch.manual_seed(seed)
    return (nets.InterNet if kind == "inter" else nets.ExtraNet)(a)


def _clip(B, T, H, W, seed):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 256, (B, T, H, W, 3)).astype(np.uint8), rng.randint(0, 20, (B, T, H, W)).astype(np.uint8))


def test_frame_scores_with_a_scorer(dev, monkeypatch):
    s = _scorer(monkeypatch, "fp32", 8)
    frames, labels = _clip(2, 4, 32, 64, 11)
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    pred, gt, pl, gl = f[:, :2], f[:, 2:], l[:, :2], l[:, 2:]  # (2, 2) strided views
    with_s = frame_scores(pred, gt, pl, gl, n_classes=NC, perceptual=s)
    without = frame_scores(pred, gt, pl, gl, n_classes=NC)
    assert without.vgg is None and with_s.vgg.shape == (2, 2) and with_s.vgg.dtype == torch.float64
    assert _bits(with_s.vgg).tobytes() == _bits(s(pred, gt)).tobytes()
    for k in ("sse", "ssim", "agree", "valid", "inter", "uni"):
        a, b = getattr(with_s, k), getattr(without, k)
        assert a.dtype == b.dtype and a.shape == b.shape and _bits(a).tobytes() == _bits(b).tobytes(), k
    with pytest.raises(ValueError):
        frame_scores(f[:, :2, :15], f[:, 2:, :15], perceptual=s)  # a side below 16


@pytest.mark.parametrize("kind", ["inter", "extra"])
def test_score_video_with_a_scorer(dev, monkeypatch, kind):
    s = _scorer(monkeypatch, "fp32", 8)
    model = _net(kind).to(dev).eval()
    frames, labels = _clip(2, 5, 32, 64, 61)
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    syn = VideoSynthesizer(model, max_batch=2)
    if kind == "inter":
        sc = syn.score_interpolation(f, l, levels=2, perceptual=s)
        plain = syn.score_interpolation(f, l, levels=2)
        truth = lambda j: f[:, sc.slots[j]]  # noqa: E731
        pred = lambda j: sc.frames[:, sc.slots[j]]  # noqa: E731
    else:
        sc = syn.score_extrapolation(f, l, perceptual=s)
        plain = syn.score_extrapolation(f, l)
        truth = lambda j: f[:, 2 + j]  # noqa: E731
        pred = lambda j: sc.frames[:, j]  # noqa: E731
    assert plain.vgg is None and "vgg" not in plain.summary() and len(plain.host()) == 4
    with pytest.raises(ValueError):
        plain.host(vgg=True)
    assert sc.vgg.shape == (2, len(sc.slots)) == (2, 3) and sc.vgg.dtype == torch.float64
    for k in ("sse", "ssim", "agree", "valid", "inter", "uni"):
        assert _bits(getattr(sc, k)).tobytes() == _bits(getattr(plain, k)).tobytes(), k
    direct = torch.stack([s(pred(j), truth(j)) for j in range(len(sc.slots))], dim=1)  # slot by slot
    assert bool(torch.isfinite(sc.vgg).all()) and float((sc.vgg - direct).abs().max()) <= GATE["fp32"]
    if kind == "extra":  # scored in one call over the (B, S) views: the same call gives the same bits
        assert _bits(sc.vgg).tobytes() == _bits(s(sc.frames, f[:, 2:])).tobytes()
    assert len(sc.host()) == 4 and len(sc.host(vgg=True)) == 5
    v, pos, summ = sc.vgg.cpu().numpy(), np.asarray(sc.positions), sc.summary()
    assert np.array_equal(sc.host(vgg=True)[4], v)
    assert summ["vgg"] == float(np.mean(v.ravel()))
    for p, row in summ["per_position"].items():
        assert row["vgg"] == float(np.mean(v[:, pos == p].ravel())), p
    base = plain.summary()
    assert {k: x for k, x in summ.items() if k not in ("vgg", "per_position")} == \
        {k: x for k, x in base.items() if k != "per_position"}


def _keys(x):
    if isinstance(x, dict):
        return set(x) | {k for v in x.values() for k in _keys(v)}
    if isinstance(x, list):
        return {k for v in x for k in _keys(v)}
    return set()


def _launch(tmp_path, dev, runner, kind, name, T, extra, tag):
    from PIL import Image
    from deep_video_interpolation_extrapolation_amd import main as M
    H, W = 32, 64
    frames, labels = _clip(1, T, H, W, 71)
    data = tmp_path / f"data_{tag}"
    for sub in ("rgb", "seg"):
        (data / sub / "aachen_000001").mkdir(parents=True)
    for t in range(T):
        Image.fromarray(frames[0, t]).save(data / "rgb" / "aachen_000001" / f"{t:02d}.png")
        Image.fromarray(labels[0, t]).save(data / "seg" / "aachen_000001" / f"{t:02d}.png")
    model = _net(kind, seed=7).to(dev).eval()
    run = tmp_path / f"run_{tag}"
    (run / "checkpoint").mkdir(parents=True)
    torch.save({"session": 0, "epoch": 2, "coarse_model": model.coarse_model.state_dict()},
               run / "checkpoint" / f"{name}_xs2xs_{kind}_0_1_0.pth")
    M.main(["--split", "test", "--synth_eval", "--syn_type", kind, "--input_h", str(H), "--input_w", str(W),
            "--precision", "fp32", "--load_dir", str(run), "--checksession", "0", "--checkepoch", "1",
            "--checkpoint", "0", "--cycgen_load_dir", str(data)] + extra + [runner, "--load_coarse"]
           + (["--num_pred_step", "2"] if runner == "EXTRA" else []))
    return json.loads((data / "synth_eval" / "scores.json").read_text()), model, frames, labels


@pytest.mark.parametrize("runner,kind,name,T,extra", [("INTER", "inter", "InterNet", 5, ["--synth_levels", "2"]),
                                                      ("EXTRA", "extra", "ExtraNet", 4, [])])
def test_main_launcher_synth_vgg(dev, monkeypatch, tmp_path, runner, kind, name, T, extra):
    got, model, frames, labels = _launch(tmp_path, dev, runner, kind, name, T, extra + ["--synth_vgg"], kind)
    s = _scorer(monkeypatch, "fp32", 8)
    f, l = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    syn = VideoSynthesizer(model, max_batch=1)
    sc = syn.score_interpolation(f, l, levels=2, perceptual=s) if runner == "INTER" else \
        syn.score_extrapolation(f, l, perceptual=s)
    row = got["clips"]["aachen_000001"]
    assert row["slots"] == sc.slots and len(row["vgg"]) == len(sc.slots)
    assert np.isfinite(row["vgg"]).all() and np.abs(np.asarray(row["vgg"]) - sc.vgg[0].cpu().numpy()).max() <= GATE["fp32"]
    for k in ("psnr", "ssim", "acc", "miou"):
        assert row[k] == getattr(sc, k)[0].cpu().numpy().tolist(), k
    assert got["summary"]["vgg"] == float(np.mean(row["vgg"]))
    pos = np.asarray(sc.positions)
    for p, r in got["summary"]["per_position"].items():
        assert r["vgg"] == float(np.mean(np.asarray(row["vgg"])[pos == int(p)])), p
    assert got["vgg_weights"] == "synthetic-seed19"


def test_main_launcher_without_synth_vgg_has_no_vgg_key(dev, tmp_path):
    got, *_ = _launch(tmp_path, dev, "INTER", "inter", "InterNet", 5, ["--synth_levels", "2"], "plain")
    assert list(got) == ["clips", "summary"]
    assert not [k for k in _keys(got) if str(k).startswith("vgg")]
    assert list(got["clips"]["aachen_000001"]) == ["slots", "psnr", "ssim", "acc", "miou"]
