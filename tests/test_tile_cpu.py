"""CPU checks of tiled synthesis: the tile plan and its argument rules, the blend weights of the numpy
restatement (tests/tile_ref.py), VideoSynthesizer.tiles and max_pixels, the options, the C ABI of
dvie_synth_tile_blend and its argument checks (no GPU: an invalid descriptor returns before any launch)."""
import ctypes
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import nets, synth
from deep_video_interpolation_extrapolation_amd.options import Options
import tile_ref as R


# ---------------- the plan ----------------
def test_plan_properties():
    """m in {4, 8, 16}, tile up to 12m, overlap in multiples of m up to tile // 2, size up to 40m"""
    count = 0
    for m in (4, 8, 16):
        for tile in range(m, 12 * m + 1, m):
            for overlap in range(0, tile // 2 + 1, m):
                for size in range(m, 40 * m + 1, m):
                    if size > tile and -(-(size - overlap) // (tile - overlap)) > 32:
                        with pytest.raises(ValueError, match="at most 32"):
                            synth.tile_starts(size, tile, overlap, m)
                        continue
                    starts, extent = synth.tile_starts(size, tile, overlap, m)
                    assert (starts, extent) == R.tile_starts(size, tile, overlap, m)
                    count += 1
                    if size <= tile:
                        assert (starts, extent) == ([0], size)
                        continue
                    assert extent == tile and starts[0] == 0 and starts[-1] + tile == size
                    assert len(starts) == -(-(size - overlap) // (tile - overlap)) >= 2
                    d = np.diff(starts)
                    assert (d > 0).all() and not (np.asarray(starts) % m).any()
                    assert (tile - d >= overlap).all()  # neighbours share at least `overlap`
                    cover = np.zeros(size, dtype=int)
                    for s in starts:
                        cover[s:s + tile] += 1
                    assert cover.min() >= 1 and cover.max() <= 3, (m, tile, overlap, size, starts)
    assert count > 5000


def test_plan_examples():
    assert synth.tile_starts(44, 24, 8, 4) == ([0, 8, 20], 24)  # three tiles over rows 20..23
    assert synth.tile_starts(72, 40, 8, 4) == ([0, 32], 40)
    assert synth.tile_starts(24, 24, 8, 4) == ([0], 24) and synth.tile_starts(16, 24, 8, 4) == ([0], 16)
    assert synth.tile_starts(2160, 1152, 64, 4) == ([0, 1008], 1152)
    assert synth.tile_starts(3840, 2048, 64, 4) == ([0, 1792], 2048)
    assert synth.tile_starts(1088, 576, 64, 4)[0] == [0, 512] and synth.tile_starts(1920, 1024, 64, 4)[0] == [0, 896]


@pytest.mark.parametrize("args,word", [
    ((44, 22, 8, 4), "tile"), ((44, 0, 0, 4), "tile"), ((44, 24, 6, 4), "overlap"), ((44, 24, 16, 4), "overlap"),
    ((44, 24, -4, 4), "overlap"), ((4096, 1024, 260, 4), "overlap"), ((42, 24, 8, 4), "size"), ((0, 24, 8, 4), "size"),
    ((44, 24, 8, 0), "m="), ((4 * 33, 4, 0, 4), "tile"), ((44.0, 24, 8, 4), "size"), ((44, 24, True, 4), "overlap"),
])
def test_plan_argument_errors(args, word):
    with pytest.raises(ValueError, match=word):
        synth.tile_starts(*args)


def test_plan_tile_count_limit():
    assert len(synth.tile_starts(4 * 32, 4, 0, 4)[0]) == 32
    assert synth.tile_starts(8192, 512, 256, 4)[1] == 512  # overlap 256 is allowed
    with pytest.raises(ValueError, match="33 tiles"):
        synth.tile_starts(4 * 33, 4, 0, 4)


# ---------------- the weights ----------------
@pytest.mark.parametrize("hp,wp,th,tw,ov,m", [(44, 72, 24, 40, 8, 4), (24, 88, 24, 40, 8, 4), (44, 72, 24, 40, 0, 4),
                                             (96, 64, 32, 32, 16, 16)])
def test_weights(hp, wp, th, tw, ov, m):
    ys, eh = R.tile_starts(hp, th, ov, m)
    xs, ew = R.tile_starts(wp, tw, ov, m)
    w = R.weights(ys, xs, eh, ew, ov)
    assert w.shape == (len(ys) * len(xs), hp, wp) and w.min() >= 0 and w.max() <= (ov + 1) ** 2
    assert (w.sum(0) > 0).all()  # every canvas pixel is covered with a positive sum
    assert ((w > 0).sum(0) <= 9).all()
    t = 0
    for y0 in ys:
        for x0 in xs:
            inside = np.zeros((hp, wp), dtype=bool)
            inside[y0:y0 + eh, x0:x0 + ew] = True
            assert (w[t][inside] >= 1).all() and not w[t][~inside].any()
            t += 1
    if ov == 0:
        assert set(np.unique(w)) <= {0, 1}  # coinciding tiles are averaged
    # canvas borders do not ramp: along a border the first / last tile's axis weight is flat
    for starts, e, S in ((ys, eh, hp), (xs, ew, wp)):
        first, last = R.axis_weights(starts[0], e, S, ov), R.axis_weights(starts[-1], e, S, ov)
        if len(starts) > 1:
            d0, d1 = starts[1], starts[-2] + e  # where the neighbour begins / ends
            assert (first[:d0] == ov + 1).all() and (last[d1:] == ov + 1).all()
            assert first[e - 1] == 1 and last[starts[-1]] == 1  # the inner edges ramp down to 1
        else:
            assert (first == ov + 1).all()


def test_reference_blend_of_equal_tiles_is_the_tile():
    """tiles cut from one map blend back to values within rounding of it, single-covered pixels bit for bit"""
    rng = np.random.RandomState(3)
    ys, xs, th, tw, ov = [0, 8, 20], [0, 32], 24, 40, 8
    full = rng.uniform(-2, 2, (2, 44, 72, 8)).astype(np.float32)
    tiles = np.stack([full[:, y:y + th, x:x + tw] for y in ys for x in xs])
    got = R.blend_map(tiles, ys, xs, ov)
    single = (R.weights(ys, xs, th, tw, ov) > 0).sum(0) == 1
    assert single.any() and not single.all()
    assert np.array_equal(got[:, single].view(np.uint32), full[:, single].view(np.uint32))
    assert np.abs(got - full).max() <= 4 * np.finfo(np.float32).eps * 2


# ---------------- the synthesiser's plan and size guard ----------------
def _args(precision="fp32", large=False, n_scales=2):
    return types.SimpleNamespace(syn_type="inter", highres_large=large, coarse_model="HRNet", precision=precision,
                                 n_scales=n_scales, stage3_prop=False, refine_model="SRNRefine",
                                 stage3_model="MSResAttnRefine")


class _Stub(synth.VideoSynthesizer):
    """a synthesiser of a given multiple without a net"""

    def __init__(self, m, pad=None, tile=None, overlap=0):
        self._m, self.pad, self.tile, self.overlap = m, pad, tile, overlap

    multiple = property(lambda self: self._m)


@pytest.mark.parametrize("m", [4, 8, 16])
def test_tiles_on_a_stub(m):
    th, tw, ov = 6 * m, 10 * m, 2 * m
    syn = _Stub(m, tile=(th, tw), overlap=ov)
    H, W = 11 * m, 18 * m
    tiles = syn.tiles(H, W)
    ys, xs = synth.tile_starts(H, th, ov, m)[0], synth.tile_starts(W, tw, ov, m)[0]
    assert tiles == [(y, x, th, tw) for y in ys for x in xs] and len(tiles) == len(ys) * len(xs) > 1
    assert syn.tiles(th, tw) == [(0, 0, th, tw)] and syn.tiles(m, 2 * m) == [(0, 0, m, 2 * m)]
    assert syn.tiles(th, W) == [(0, x, th, tw) for x in xs]  # only the columns are tiled
    assert _Stub(m).tiles(H, W) == [(0, 0, H, W)]
    # with pad the tiles are those of the canvas
    padded = _Stub(m, pad="replicate", tile=(th, tw), overlap=ov)
    assert padded.tiles(H - m + 1, W - 1) == tiles and padded.tiles(H - m, W) == syn.tiles(H - m, W)
    assert padded.tiles(1, 1) == [(0, 0, m, m)]


def test_constructor_arguments():
    net = nets.InterNet(_args())
    syn = synth.VideoSynthesizer(net)
    assert syn.tile is None and syn.tiles(44, 72) == [(0, 0, 44, 72)]
    syn = synth.VideoSynthesizer(net, tile=(24, 40), overlap=8)
    assert syn.tile == (24, 40) and syn.overlap == 8 and len(syn.tiles(44, 72)) == 6
    assert synth.VideoSynthesizer(net, tile=(576, 1024)).overlap == 64
    for bad in ((22, 40), (24, 42), (24,), "24x40", (0, 40), (24.0, 40)):
        with pytest.raises(ValueError, match="multiple 4"):
            synth.VideoSynthesizer(net, tile=bad, overlap=8)
    with pytest.raises(ValueError, match="multiple 8"):
        synth.VideoSynthesizer(nets.InterNet(_args(large=True)), tile=(28, 40), overlap=8)
    for bad in (6, 16, -4, 64):  # no multiple; more than half of the smaller side; negative; the default on a small tile
        with pytest.raises(ValueError, match="overlap"):
            synth.VideoSynthesizer(net, tile=(24, 40), overlap=bad)


def test_max_pixels_and_the_size_guard():
    UHD, HD = (2160, 3840), (1088, 1920)
    bf16 = synth.VideoSynthesizer(nets.InterNet(_args("bf16")))
    fp32 = synth.VideoSynthesizer(nets.InterNet(_args("fp32")))
    # the head's concat: 448 channels of 2 / 4 bytes against 0xFFFFFF00, strictly below
    assert bf16.max_pixels == (0xFFFFFF00 - 1) // (448 * 2) == 4793489
    assert fp32.max_pixels == (0xFFFFFF00 - 1) // (448 * 4) == bf16.max_pixels // 2
    assert UHD[0] * UHD[1] > bf16.max_pixels >= HD[0] * HD[1] and fp32.max_pixels >= HD[0] * HD[1]
    bf16._check_size(*HD)
    fp32._check_size(*HD)
    for syn in (bf16, fp32):
        with pytest.raises(synth.FrameSizeError, match=r"tile=") as e:
            syn._check_size(*UHD)
        assert e.value.too_large and "2160x3840" in str(e.value) and str(syn.max_pixels) in str(e.value)
    # tiled: the tile shape is what counts
    tiled = synth.VideoSynthesizer(nets.InterNet(_args("bf16")), tile=(1152, 2048))
    tiled._check_size(*UHD)
    assert tiled.tiles(*UHD) == [(0, 0, 1152, 2048), (0, 1792, 1152, 2048), (1008, 0, 1152, 2048), (1008, 1792, 1152, 2048)]
    too_big = synth.VideoSynthesizer(nets.InterNet(_args("bf16")), tile=(2160, 2400))
    with pytest.raises(synth.FrameSizeError, match=r"a tile of 2160x2400.*tile="):
        too_big._check_size(*UHD)
    too_big._check_size(*HD)  # (the canvas fits: one forward of the canvas)
    # the stages of a two-stage net are narrower than HRNet's concat; highres_large's concat is wider
    assert synth.VideoSynthesizer(nets.InterStage3Net(_args("bf16"))).max_pixels == bf16.max_pixels
    assert synth.VideoSynthesizer(nets.InterNet(_args("bf16", large=True))).max_pixels < bf16.max_pixels


def test_launcher_hint_names_the_flag():
    from deep_video_interpolation_extrapolation_amd.runners.InterTrainer import InterTrainer
    big = synth.FrameSizeError("a forward of too many pixels: pass tile=(th, tw)")
    big.too_large = True
    out = InterTrainer._size_hint(big)
    assert isinstance(out, synth.FrameSizeError) and out.too_large and "--synth_tile" in str(out) and "tile=" in str(out)
    out = InterTrainer._size_hint(synth.FrameSizeError("H and W must be multiples of 4, got (13, 30)"))
    assert "--synth_pad replicate" in str(out) and "--synth_tile" not in str(out)


# ---------------- options ----------------
def test_options_synth_tile(capsys):
    a = Options().parse(["INTER"])
    assert a.synth_tile is None and a.synth_tile_overlap == 64
    a = Options().parse(["--synth_tile", "576x1024", "--synth_tile_overlap", "32", "INTER"])
    assert a.synth_tile == (576, 1024) and a.synth_tile_overlap == 32
    a = Options().parse(["--synth_tile", "24x40", "--synth_tile_overlap", "0", "EXTRA"])
    assert a.synth_tile == (24, 40) and a.synth_tile_overlap == 0
    for flag, bad in (("--synth_tile", "576"), ("--synth_tile", "576x"), ("--synth_tile", "576X1024"), ("--synth_tile", "0x64"),
                      ("--synth_tile", "24x40x3"), ("--synth_tile", " 24x40"), ("--synth_tile", "-24x40"),
                      ("--synth_tile", "24.0x40"), ("--synth_tile_overlap", "-8"), ("--synth_tile_overlap", "8.0"),
                      ("--synth_tile_overlap", "x")):
        with pytest.raises(SystemExit):
            Options().parse([flag, bad, "INTER"])
        assert flag in capsys.readouterr().err
    # a well-formed value that is no multiple: the constructor's ValueError names the net's multiple
    a = Options().parse(["--synth_tile", "22x40", "--synth_tile_overlap", "8", "INTER"])
    with pytest.raises(ValueError, match="multiple 4"):
        synth.VideoSynthesizer(nets.InterNet(_args()), tile=a.synth_tile, overlap=a.synth_tile_overlap)


# ---------------- C ABI ----------------
def test_symbol_and_descriptor_size():
    lib = L.load()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dvie_[a-z0-9_]+)", out))
    assert "dvie_synth_tile_blend" in exported and "dvie_synth_tile_blend" in L.EXPORTS and hasattr(lib, "dvie_synth_tile_blend")
    assert L._ABI_MORE[115] is L.SynthTileBlendDesc and L.TILE_MAX == synth.TILE_MAX == 32
    assert lib.dvie_abi_sizeof(115) == ctypes.sizeof(L.SynthTileBlendDesc) == 6 * 8 + 14 * 4 + 2 * 32 * 4
    assert lib.dvie_abi_sizeof(116) == 0


def _desc(**kw):
    """a valid descriptor: canvas 44x72 from 3 x 2 tiles of 24x40, a crop of 41x70 (the pointers are never followed)"""
    d = L.SynthTileBlendDesc()
    base = dict(rgb_tiles=64, seg_tiles=64, rgb_out=64, frame=65, label=67, label_canvas=66, n=2, th=24, tw=40, hp=44, wp=72,
                h=41, w=70, rgb_ld=8, seg_ld=24, n_classes=20, overlap=8, nty=3, ntx=2, ys=[0, 8, 20], xs=[0, 32])
    base.update(kw)
    for k, v in base.items():
        if k in ("ys", "xs"):
            for i, s in enumerate(v):
                getattr(d, k)[i] = s
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,word", [
    (dict(rgb_tiles=None), b"null"), (dict(seg_tiles=None), b"null"), (dict(frame=None), b"null"), (dict(label=None), b"null"),
    (dict(rgb_ld=6), b"multiples of 4"), (dict(seg_ld=22), b"multiples of 4"), (dict(rgb_ld=0), b"multiples of 4"),
    (dict(rgb_tiles=68), b"aligned"), (dict(seg_tiles=72), b"aligned"), (dict(rgb_out=72), b"aligned"),
    (dict(ys=[0, 20, 8]), b"increase"), (dict(ys=[0, 8, 8]), b"increase"), (dict(xs=[0, 0]), b"increase"),
    (dict(ys=[0, 8, 24]), b"leaves the canvas"), (dict(xs=[0, 36]), b"leaves the canvas"), (dict(th=48), b"leaves the canvas"),
    (dict(ys=[4, 8, 20]), b"do not cover"), (dict(nty=2), b"do not cover"), (dict(ntx=1), b"do not cover"),
    (dict(th=8, nty=2, ys=[0, 36]), b"do not cover"), (dict(xs=[0, 28]), b"do not cover"),
    (dict(h=45), b"h=45"), (dict(w=73), b"w=73"), (dict(h=0), b"h=0"),
    (dict(n_classes=25), b"n_classes"), (dict(n_classes=0), b"n_classes"), (dict(seg_ld=512, n_classes=257), b"n_classes"),
    (dict(overlap=257), b"overlap"), (dict(overlap=-1), b"overlap"),
    (dict(nty=0), b"per axis"), (dict(ntx=33), b"per axis"), (dict(n=0), b"n=0"),
])
def test_tile_blend_argument_validation_without_gpu(kw, word):
    lib = L.load()
    assert lib.dvie_synth_tile_blend(ctypes.byref(_desc(**kw)), None) == L.DVIE_EINVAL, kw
    assert word in lib.dvie_last_error(), (kw, lib.dvie_last_error())


def test_null_descriptor_and_cpu_tensors():
    lib = L.load()
    assert lib.dvie_synth_tile_blend(None, None) == L.DVIE_EINVAL and b"null" in lib.dvie_last_error()
    z = torch.zeros
    with pytest.raises(L.DvieError):
        synth.tile_blend(z((2, 1, 8, 8, 8)), z((2, 1, 8, 8, 24)), [0], [0, 4], 4, z((1, 8, 12, 3), dtype=torch.uint8),
                         z((1, 8, 12), dtype=torch.uint8))
