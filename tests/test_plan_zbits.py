"""Plan compiler, CPU (descriptor lists are built; nothing is launched): activation sign
bitmaps (include/dvie.h dvie_conv_desc.zbits).  HRNet (bf16, as a training plan) and the
VGG19 loss plan are lowered at 16x16 and compiled on the CPU:
* a backward descriptor with a bitmap carries a ReLU / LeakyReLU derivative, and its
  (zbits, zbits_ld) address the bitmap of exactly one forward descriptor, the one that writes
  the z it would otherwise read;
* every descriptor with a bitmap is one whose kernel honours it (dvie_conv_zbits), so no
  bitmap is written that nobody reads and none is read that nobody wrote;
* DVIE_ZBITS=0 compiles the same lists without any;
* a bitmap is a tensor of its own, n * H * W * C / 8 bytes, sharing no storage with an
  activation or gradient buffer; z / z_ld stay set next to it;
* the algorithmic bytes (profiling meta) of a reader drop by the 2 bytes - 1 bit per element."""
import ctypes
import types

import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import engine as E
from deep_video_interpolation_extrapolation_amd import nets
from deep_video_interpolation_extrapolation_amd.nets.vgg import my_vgg, vgg19_features

SIGN = (L.ACT_LRELU, L.ACT_RELU)
CPU = torch.device("cpu")


def _plans():
    torch.manual_seed(1024)
    a = types.SimpleNamespace(syn_type="inter", highres_large=False, coarse_model="HRNet")
    hr = nets.InterNet(a).coarse_model
    g = hr._lower(E.Graph(torch.bfloat16), 16, 16, vgrad=True)
    gv = E.Graph(torch.bfloat16)
    my_vgg(vgg19_features()).lower(gv, 16, 16, True, True)
    return [g.compile(2, CPU, backward=True), gv.compile(4, CPU, n_bwd=2, backward=True)]


def _convs(ops):
    return [o for o in ops if o.kind == L.OP_CONV]


@pytest.fixture(scope="module")
def plans_on():
    mp = pytest.MonkeyPatch()
    mp.setenv("DVIE_ZBITS", "1")
    try:
        yield _plans()
    finally:
        mp.undo()


def test_bitmaps_pair_one_writer_with_its_readers(plans_on):
    lib = L.load()
    n_readers = 0
    for plan in plans_on:
        writers = [o for o in _convs(plan.fwd) if o.u.conv.zbits]
        readers = [o for o in _convs(plan.bwd) if o.u.conv.zbits]
        for o in writers:
            d = o.u.conv
            assert d.act in SIGN and d.dact == 0 and d.zbits_ld * 8 == d.y_ld, o.meta["name"]
            assert lib.dvie_conv_zbits(ctypes.byref(d)) == 1, o.meta["name"]
        read_of = {id(o): 0 for o in writers}
        for o in readers:
            d = o.u.conv
            assert d.dact in SIGN and d.z and d.z_ld == 8 * d.zbits_ld, o.meta["name"]
            assert lib.dvie_conv_zbits(ctypes.byref(d)) == 1, o.meta["name"]
            # the writer of the z this descriptor would read: same pixel row, the bitmap
            # offset is the channel offset / 8 (z in bf16: byte offset / 16)
            mine = [f for f in writers if f.u.conv.zbits_ld == d.zbits_ld and f.u.conv.y_ld == d.z_ld
                    and 0 <= d.z - f.u.conv.y < 2 * d.z_ld and d.z - f.u.conv.y == 16 * (d.zbits - f.u.conv.zbits)]
            assert len(mine) == 1, (o.meta["name"], [f.meta["name"] for f in mine])
            read_of[id(mine[0])] += 1
        assert all(read_of.values()), "a bitmap is written that no data gradient reads"
        assert len(writers) == len(plan.zbits)
        n_readers += len(readers)
    # layer1's 256-channel block outputs: 1x1 producer (conv3 + residual + ReLU) and 1x1 reader
    # (the next block's conv1 data gradient) are covered at any size
    assert {"layer1.0.out", "layer1.1.out", "layer1.2.out"} <= set(plans_on[0].zbits), sorted(plans_on[0].zbits)
    assert n_readers >= 3


def test_bitmaps_are_tensors_of_their_own(plans_on):
    for plan in plans_on:
        stor = set()
        for b in plan.g.buffers:
            for t in (b.t, b.g):
                if t is not None:
                    stor.add(t.untyped_storage().data_ptr())
        by_name = {b.name: b for b in plan.g.buffers}
        for name, t in plan.zbits.items():
            b = by_name[name]
            assert t.dtype == torch.uint8 and t.numel() == plan.nf * b.H * b.W * b.C // 8
            assert t.untyped_storage().data_ptr() not in stor
            assert t.untyped_storage().nbytes() == t.numel() and any(k is t for k in plan.keep)


def test_switch_compiles_plans_without_bitmaps(plans_on, monkeypatch):
    monkeypatch.setenv("DVIE_ZBITS", "0")
    plans_off = _plans()
    for on, off in zip(plans_on, plans_off):
        assert not off.zbits
        assert not [o for o in _convs(off.fwd + off.bwd) if o.u.conv.zbits or o.u.conv.zbits_ld]
        assert [o.kind for o in on.fwd] == [o.kind for o in off.fwd]
        assert [o.kind for o in on.bwd] == [o.kind for o in off.bwd]
        for a, b in zip(on.bwd, off.bwd):
            if a.kind != L.OP_CONV:
                continue
            d = a.u.conv
            assert (d.dact, d.z_ld, d.beta, bool(d.z), bool(d.res)) == (
                b.u.conv.dact, b.u.conv.z_ld, b.u.conv.beta, bool(b.u.conv.z), bool(b.u.conv.res))
            if d.zbits:  # 2 bytes per element of z give way to 1 bit
                assert a.meta["bytes"] == b.meta["bytes"] - d.n * d.oh * d.ow * d.cout * (2 - 0.125), a.meta["name"]
            else:
                assert a.meta["bytes"] == b.meta["bytes"]
