"""CPU checks of the self-ensemble: the member table, the constructor rules, the option, the C ABI of
dvie_synth_flip / dvie_synth_ens_acc and their argument checks (no GPU: an invalid descriptor returns
before any launch)."""
import ctypes
import re
import subprocess
import types

import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import nets, synth
from deep_video_interpolation_extrapolation_amd.options import Options

SETTINGS = {None: [(0, 0)], "time": [(0, 0), (1, 0)], "flip": [(0, 0), (0, 1)],
            "time+flip": [(0, 0), (1, 0), (0, 1), (1, 1)]}


def _args(kind="inter"):
    return types.SimpleNamespace(syn_type=kind, highres_large=False, coarse_model="HRNet", precision="fp32",
                                 n_scales=2, stage3_prop=False, refine_model="SRNRefine", stage3_model="MSResAttnRefine")


# ---------------- the members ----------------
def test_members_and_their_order():
    for setting, want in SETTINGS.items():
        got = synth.ensemble_members(setting)
        assert [tuple(m) for m in got] == want, setting
        assert got[0] == (0, 0) and len(got) in (1, 2, 4)  # the plain forward first; 1 / M is exact
    got = synth.ensemble_members("time")
    got.append((1, 1))  # (a caller's list: the table itself is not handed out)
    assert synth.ensemble_members("time") == [(0, 0), (1, 0)]


@pytest.mark.parametrize("bad", ["none", "flip+time", "vflip", "", "TIME", 2, ("time",), True])
def test_unknown_settings_name_the_choices(bad):
    with pytest.raises(ValueError) as e:
        synth.ensemble_members(bad)
    for word in ("None", '"time"', '"flip"', '"time+flip"'):
        assert word in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="time\\+flip"):
        synth.VideoSynthesizer(nets.InterNet(_args()), ensemble=bad)


def test_constructor_rules():
    inter = nets.InterNet(_args())
    assert synth.VideoSynthesizer(inter).ensemble is None and synth.VideoSynthesizer(inter).members == [(0, 0)]
    for setting, want in SETTINGS.items():
        syn = synth.VideoSynthesizer(inter, ensemble=setting)
        assert syn.ensemble == setting and syn.members == want
    assert synth.VideoSynthesizer(nets.InterStage3Net(_args()), ensemble="time+flip").members == SETTINGS["time+flip"]
    for name in ("ExtraNet", "ExtraRefineNet", "ExtraStage3Net"):
        extra = nets.__dict__[name](_args("extra"))
        for setting in ("time", "time+flip"):
            with pytest.raises(ValueError, match="extrapolation has no time symmetry"):
                synth.VideoSynthesizer(extra, ensemble=setting)
        assert synth.VideoSynthesizer(extra, ensemble="flip").members == [(0, 0), (0, 1)]
        assert synth.VideoSynthesizer(extra).members == [(0, 0)]


# ---------------- the option ----------------
def test_options_synth_ensemble(capsys):
    assert Options().parse(["INTER"]).synth_ensemble == "none"
    assert Options().parse(["--split", "test", "EXTRA"]).synth_ensemble == "none"
    for choice in ("none", "time", "flip", "time+flip"):
        assert Options().parse(["--split", "test", "--synth_ensemble", choice, "INTER"]).synth_ensemble == choice
    assert Options().parse(["--synth_ensemble", "flip", "--synth_eval", "EXTRA"]).synth_ensemble == "flip"
    for bad in ("flip+time", "vflip", "TIME", "1"):
        with pytest.raises(SystemExit):
            Options().parse(["--synth_ensemble", bad, "INTER"])
        assert "--synth_ensemble" in capsys.readouterr().err


def test_wrappers_refuse_cpu_tensors():
    z = torch.zeros
    with pytest.raises(L.DvieError):
        synth.synth_flip(z((1, 2, 4, 8)), z((1, 2, 4), dtype=torch.uint8), z((1, 2, 4, 8)), z((1, 2, 4), dtype=torch.uint8))
    with pytest.raises(L.DvieError):
        synth.synth_ens_acc(z((1, 2, 4, 8)), z((1, 2, 4, 24)), z((1, 2, 4, 8)), z((1, 2, 4, 24)), flip=True, last_m=2)


# ---------------- C ABI ----------------
def test_symbols_and_descriptor_sizes():
    lib = L.load()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dvie_[a-z0-9_]+)", out))
    for name in ("dvie_synth_flip", "dvie_synth_ens_acc"):
        assert name in exported and name in L.EXPORTS and hasattr(lib, name), name
    assert L._ABI_MORE[118] is L.SynthFlipDesc and L._ABI_MORE[119] is L.SynthEnsAccDesc
    assert lib.dvie_abi_sizeof(118) == ctypes.sizeof(L.SynthFlipDesc) == 4 * 8 + 2 * 8 + 4 * 4
    assert lib.dvie_abi_sizeof(119) == ctypes.sizeof(L.SynthEnsAccDesc) == 4 * 8 + 10 * 4
    assert lib.dvie_abi_sizeof(120) == 0


def _flip(**kw):
    """a valid descriptor: two 3x5 images of 8 channels and their label maps (the pointers are never followed)"""
    d = L.SynthFlipDesc()
    base = dict(src=4096, dst=8192, lsrc=12289, ldst=12401, src_stride=120, lsrc_stride=15, n=2, h=3, w=5, ld=8)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def _acc(**kw):
    d = L.SynthEnsAccDesc()
    base = dict(rgb=4096, seg=8192, rgb_acc=16384, seg_acc=32768, n=2, h=3, w=5, rgb_ld=8, seg_ld=24, n_classes=20,
                flip=1, first=0, last_m=2)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("fn,desc,kw,word", [
    ("dvie_synth_flip", _flip, dict(src=None), b"null"), ("dvie_synth_flip", _flip, dict(dst=None), b"null"),
    ("dvie_synth_flip", _flip, dict(w=0), b"w=0"), ("dvie_synth_flip", _flip, dict(h=0), b"h=0"),
    ("dvie_synth_flip", _flip, dict(n=0), b"n=0"), ("dvie_synth_flip", _flip, dict(ld=6), b"multiple of 4"),
    ("dvie_synth_flip", _flip, dict(ld=0), b"multiple of 4"),
    ("dvie_synth_flip", _flip, dict(dst=4096), b"src == dst"), ("dvie_synth_flip", _flip, dict(ldst=12289), b"lsrc == ldst"),
    ("dvie_synth_flip", _flip, dict(dst=4096 + 64), b"overlap"), ("dvie_synth_flip", _flip, dict(ldst=12289 + 7), b"overlap"),
    ("dvie_synth_flip", _flip, dict(lsrc=None), b"both or neither"), ("dvie_synth_flip", _flip, dict(ldst=None), b"both or neither"),
    ("dvie_synth_flip", _flip, dict(src=4100), b"aligned"), ("dvie_synth_flip", _flip, dict(src_stride=119), b"src_stride"),
    ("dvie_synth_flip", _flip, dict(src_stride=64), b"src_stride"), ("dvie_synth_flip", _flip, dict(lsrc_stride=14), b"lsrc_stride"),
    ("dvie_synth_ens_acc", _acc, dict(rgb=None), b"null"), ("dvie_synth_ens_acc", _acc, dict(seg=None), b"null"),
    ("dvie_synth_ens_acc", _acc, dict(rgb_acc=None), b"null"), ("dvie_synth_ens_acc", _acc, dict(seg_acc=None), b"null"),
    ("dvie_synth_ens_acc", _acc, dict(w=0), b"w=0"), ("dvie_synth_ens_acc", _acc, dict(rgb_ld=6), b"multiples of 4"),
    ("dvie_synth_ens_acc", _acc, dict(seg_ld=22), b"multiples of 4"),
    ("dvie_synth_ens_acc", _acc, dict(last_m=3), b"last_m=3"), ("dvie_synth_ens_acc", _acc, dict(last_m=1), b"last_m=1"),
    ("dvie_synth_ens_acc", _acc, dict(last_m=-2), b"last_m=-2"),
    ("dvie_synth_ens_acc", _acc, dict(n_classes=25), b"n_classes=25"), ("dvie_synth_ens_acc", _acc, dict(n_classes=0), b"n_classes=0"),
    ("dvie_synth_ens_acc", _acc, dict(flip=2), b"flip=2"), ("dvie_synth_ens_acc", _acc, dict(first=-1), b"first=-1"),
    ("dvie_synth_ens_acc", _acc, dict(rgb_acc=4096), b"overlap"), ("dvie_synth_ens_acc", _acc, dict(seg_acc=8192 + 16), b"overlap"),
    ("dvie_synth_ens_acc", _acc, dict(seg=8196), b"aligned"),
])
def test_argument_validation_without_gpu(fn, desc, kw, word):
    lib = L.load()
    assert getattr(lib, fn)(ctypes.byref(desc(**kw)), None) == L.DVIE_EINVAL, kw
    assert word in lib.dvie_last_error(), (kw, lib.dvie_last_error())


def test_null_descriptors():
    lib = L.load()
    assert lib.dvie_synth_flip(None, None) == L.DVIE_EINVAL and b"null" in lib.dvie_last_error()
    assert lib.dvie_synth_ens_acc(None, None) == L.DVIE_EINVAL and b"null" in lib.dvie_last_error()
