"""CPU checks of padded-canvas synthesis: the canvas size and the multiple it rounds to, the
constructor's `pad` argument, the --synth_pad flag, and the argument validation of
dvie_synth_load_pad / dvie_synth_finish_crop.  Nothing is launched."""
import ctypes
import types

import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import nets
from deep_video_interpolation_extrapolation_amd.options import Options
from deep_video_interpolation_extrapolation_amd.synth import VideoSynthesizer, canvas_size


def _args(**kw):
    a = types.SimpleNamespace(syn_type="inter", highres_large=False, coarse_model="HRNet", precision="fp32",
                              n_scales=2, stage3_prop=False, refine_model="SRNRefine", stage3_model="MSResAttnRefine")
    a.__dict__.update(kw)
    torch.manual_seed(3)
    return a


def test_canvas_size():
    assert canvas_size(150, 150, 4) == (152, 152)
    assert canvas_size(1080, 1920, 16) == (1088, 1920)
    assert canvas_size(13, 30, 4) == (16, 32)
    assert canvas_size(17, 33, 8) == (24, 40)
    assert canvas_size(1, 1, 4) == (4, 4)
    for m in (4, 8, 16):  # aligned sizes map to themselves
        for H, W in ((m, m), (2 * m, 5 * m), (1088, 1920)):
            assert canvas_size(H, W, m) == (H, W)


@pytest.mark.parametrize("make,want", [
    (lambda: nets.InterNet(_args()), 4),
    (lambda: nets.ExtraNet(_args(syn_type="extra")), 4),
    (lambda: nets.InterNet(_args(highres_large=True)), 8),
    (lambda: nets.InterRefineNet(_args(n_scales=2)), 8),
    (lambda: nets.InterRefineNet(_args(n_scales=3)), 16),
    (lambda: nets.InterStage3Net(_args(n_scales=1)), 4),
], ids=["hrnet", "extra", "highres_large", "refine_sc2", "refine_sc3", "stage3_sc1"])
def test_multiple_and_canvas_of_a_synthesizer(make, want):
    syn = VideoSynthesizer(make(), pad="replicate")
    assert syn.multiple == want
    assert syn.canvas(150, 150) == canvas_size(150, 150, want)
    assert syn.canvas(1080, 1920) == canvas_size(1080, 1920, want)
    assert syn.canvas(4 * want, 3 * want) == (4 * want, 3 * want)
    assert VideoSynthesizer(syn.net).multiple == want  # the multiple does not depend on pad


def test_pad_argument():
    net = nets.InterNet(_args())
    assert VideoSynthesizer(net).pad is None
    assert VideoSynthesizer(net, pad=None).pad is None
    assert VideoSynthesizer(net, max_batch=2, graph=False, pad="replicate").pad == "replicate"
    for bad in ("reflect", "none", "", "Replicate", 0, True):
        with pytest.raises(ValueError, match="pad"):
            VideoSynthesizer(net, pad=bad)


def test_synth_pad_flag():
    assert Options().parse(["INTER"]).synth_pad == "none"
    assert Options().parse(["--synth_pad", "replicate", "EXTRA"]).synth_pad == "replicate"
    assert Options().parse(["--synth_pad", "none", "INTER"]).synth_pad == "none"
    with pytest.raises(SystemExit):
        Options().parse(["--synth_pad", "reflect", "INTER"])


def test_new_entry_points_are_exported():
    lib = L.load()
    for name in ("dvie_synth_load_pad", "dvie_synth_finish_crop"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.dvie_abi_sizeof(108) == ctypes.sizeof(L.SynthLoadPadDesc)
    assert lib.dvie_abi_sizeof(109) == ctypes.sizeof(L.SynthFinishCropDesc)


def _call(fn, desc, base, kw):
    d = desc()
    for k, v in {**base, **kw}.items():
        setattr(d, k, v)
    return fn(ctypes.byref(d), None)


def test_load_pad_argument_validation_without_gpu():
    """dvie_synth_load_pad rejects bad descriptors before any launch"""
    lib = L.load()
    base = dict(frames=64, labels=64, out=64, label_out=64, n=2, h=13, w=30, hp=16, wp=32, out_ld=8)
    for kw, word in ((dict(frames=None), b"null"), (dict(out=None), b"null"),
                     (dict(labels=None), b"together"), (dict(label_out=None), b"together"),
                     (dict(n=0), b"n=0"),
                     (dict(h=0), b"h=0"), (dict(h=17), b"h=17"), (dict(hp=0), b"hp=0"),
                     (dict(w=0), b"w=0"), (dict(w=33), b"w=33"), (dict(wp=-4), b"wp=-4"),
                     (dict(out_ld=6), b"multiple of 4"), (dict(out_ld=0), b"multiple of 4"), (dict(out=72), b"aligned"),
                     (dict(n=1 << 20, h=4096, hp=4096), b"grid"),  # n * hp = 2**32 block rows
                     (dict(w=30, wp=1 << 24, out_ld=8), b"grid")):  # 2**17 chunks of a row
        assert _call(lib.dvie_synth_load_pad, L.SynthLoadPadDesc, base, kw) == L.DVIE_EINVAL, kw
        assert word in lib.dvie_last_error(), (kw, lib.dvie_last_error())
    assert lib.dvie_synth_load_pad(None, None) == L.DVIE_EINVAL


def test_finish_crop_argument_validation_without_gpu():
    """dvie_synth_finish_crop rejects bad descriptors before any launch"""
    lib = L.load()
    base = dict(rgb=64, seg=64, frame=65, label=67, label_canvas=None, n=2, h=13, w=30, hp=16, wp=32, rgb_ld=8,
                seg_ld=24, n_classes=20)
    for kw, word in ((dict(rgb=None), b"null"), (dict(seg=None), b"null"), (dict(frame=None), b"null"),
                     (dict(label=None), b"null"),
                     (dict(n=0), b"n=0"),
                     (dict(h=0), b"h=0"), (dict(h=17), b"h=17"), (dict(w=0), b"w=0"), (dict(w=33), b"w=33"),
                     (dict(wp=30), b"multiple of 4"), (dict(w=33, wp=34), b"multiple of 4"),
                     (dict(rgb_ld=6), b"multiples of 4"), (dict(seg_ld=22), b"multiples of 4"),
                     (dict(rgb_ld=0), b"multiples of 4"),
                     (dict(rgb=72), b"aligned"), (dict(seg=68), b"aligned"),
                     (dict(n_classes=0), b"n_classes"), (dict(n_classes=28), b"n_classes"),
                     (dict(n_classes=300, seg_ld=304), b"n_classes"),
                     (dict(n=1 << 20, h=4096, hp=4096), b"grid"),
                     (dict(wp=1 << 25), b"grid")):
        assert _call(lib.dvie_synth_finish_crop, L.SynthFinishCropDesc, base, kw) == L.DVIE_EINVAL, kw
        assert word in lib.dvie_last_error(), (kw, lib.dvie_last_error())
    assert lib.dvie_synth_finish_crop(None, None) == L.DVIE_EINVAL
