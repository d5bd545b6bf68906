"""Chained 1x1 launches (include/dvie.h dvie_conv_chain / dvie_ops_chain_pairs), host side only:
descriptor lists are built on the CPU and nothing is launched.

Plans.  HRNet (bf16, training) and the VGG19 loss plan are compiled at 16x16 and
dvie_ops_chain_pairs runs over fwd_arr and bwd_arr:
* forward: exactly layer1.N.conv3 with layer1.N+1.conv1 for N = 0, 1, 2, adjacent ops;
* backward: the layer1.N+1.conv1 data gradient with the layer1.N.conv3 data gradient wherever
  only weight-lane ops stand between them.  That holds for N = 1, 2 (one weight gradient
  between).  For N = 0 the plan has a lane-0 copy between the two (layer1.0.out's gradient also
  goes to the downsample branch, and that identity has no kernel to ride on), so by the pairing
  rule -- the next op of the caller's stream must be the partner -- that pair runs as two
  launches; the test pins the reason.  (The issue that introduced the chain expected three
  backward pairs; the plan compiler's op order, which that change leaves alone, gives two.)
* the VGG plan, an fp32 HRNet plan and DVIE_CHAIN=0 give no pair;
* partners are mutual, in range, and no op is in two pairs.
Refusals: the descriptor pairs tests/test_gpu_chain.py runs unfused are built here on host
memory addresses and dvie_conv_chain says 0 for each, 1 for the pair they were derived from."""
import ctypes
import types

import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import engine as E
from deep_video_interpolation_extrapolation_amd import nets
from deep_video_interpolation_extrapolation_amd.nets.vgg import my_vgg, vgg19_features

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def _chain_on(monkeypatch):
    monkeypatch.setenv("DVIE_CHAIN", "1")
    monkeypatch.setenv("DVIE_ZBITS", "1")


def _hrnet_plan(dtype):
    torch.manual_seed(1024)
    a = types.SimpleNamespace(syn_type="inter", highres_large=False, coarse_model="HRNet")
    hr = nets.InterNet(a).coarse_model
    g = hr._lower(E.Graph(dtype), 16, 16, vgrad=True)
    return g.compile(2, CPU, backward=True)


def _vgg_plan():
    gv = E.Graph(torch.bfloat16)
    my_vgg(vgg19_features()).lower(gv, 16, 16, True, True)
    return gv.compile(4, CPU, n_bwd=2, backward=True)


def _pairs(arr):
    """[(i, j)] with i < j, after checking the partner table itself"""
    n = len(arr)
    partner = (ctypes.c_int * n)(*([7] * n))
    count = L.load().dvie_ops_chain_pairs(arr, n, partner)
    out = []
    for i in range(n):
        j = partner[i]
        assert j == -1 or (0 <= j < n and j != i and partner[j] == i), (i, j)
        if j > i:
            out.append((i, j))
    assert count == len(out)
    assert len({k for p in out for k in p}) == 2 * len(out)
    return out


def _names(plan, arr, ops, off, pairs):
    """pairs as (name of a, name of b); off = ops of arr ahead of the Python list"""
    return [(ops[i - off].meta["name"], ops[j - off].meta["name"]) for i, j in pairs]


@pytest.fixture(scope="module")
def hrnet():
    mp = pytest.MonkeyPatch()
    mp.setenv("DVIE_ZBITS", "1")
    try:
        yield _hrnet_plan(torch.bfloat16)
    finally:
        mp.undo()


def test_hrnet_forward_pairs(hrnet):
    off = len(hrnet.fwd_arr) - len(hrnet.fwd)
    pairs = _pairs(hrnet.fwd_arr)
    assert _names(hrnet, hrnet.fwd_arr, hrnet.fwd, off, pairs) == [
        (f"layer1.{n}.conv3", f"layer1.{n + 1}.conv1") for n in range(3)]
    for i, j in pairs:
        assert j == i + 1
        assert hrnet.fwd[i - off].meta["cls"] == "conv_fwd" and hrnet.fwd[j - off].meta["cls"] == "conv_fwd"


def test_hrnet_backward_pairs(hrnet):
    arr, ops = hrnet.bwd_arr, hrnet.bwd
    assert len(arr) == len(ops)
    pairs = _pairs(arr)
    for i, j in pairs:
        assert ops[i].meta["cls"] == "conv_dgrad" and ops[j].meta["cls"] == "conv_dgrad"
        assert j > i + 1 and all(arr[k].lane == 1 for k in range(i + 1, j)), (i, j)
        assert any(arr[k].kind == L.OP_WGRAD for k in range(i + 1, j))
    assert _names(hrnet, arr, ops, 0, pairs) == [(f"layer1.{n + 1}.conv1", f"layer1.{n}.conv3") for n in (2, 1)]
    # N = 0: the descriptors would chain, but the next lane-0 op after a is a copy, not b
    dg = {o.meta["name"]: k for k, o in enumerate(ops) if getattr(o, "meta", {}).get("cls") == "conv_dgrad"}
    i, j = dg["layer1.1.conv1"], dg["layer1.0.conv3"]
    assert i < j
    assert L.load().dvie_conv_chain(ctypes.byref(arr[i].u.conv), ctypes.byref(arr[j].u.conv)) == 1
    lane0 = [k for k in range(i + 1, j) if arr[k].lane == 0]
    assert len(lane0) == 1 and arr[lane0[0]].kind == L.OP_EW and arr[lane0[0]].u.ew.op == L.EW_COPY


def test_plans_without_pairs(monkeypatch):
    vgg = _vgg_plan()
    assert _pairs(vgg.fwd_arr) == [] and _pairs(vgg.bwd_arr) == []
    f32 = _hrnet_plan(torch.float32)
    assert _pairs(f32.fwd_arr) == [] and _pairs(f32.bwd_arr) == []


def test_switch_gives_no_pairs(hrnet, monkeypatch):
    assert len(_pairs(hrnet.fwd_arr)) == 3
    monkeypatch.setenv("DVIE_CHAIN", "0")
    assert _pairs(hrnet.fwd_arr) == [] and _pairs(hrnet.bwd_arr) == []


# ---------------- the refusal table, on host addresses ----------------
def chain_descs(base, n, h, w, c=64, mid=256, cout=64, res=True, act=L.ACT_LRELU, bits=True):
    """The forward pair (a: c -> mid with bias-free residual + activation + bitmap, b: mid ->
    cout with LeakyReLU) over disjoint 16-byte aligned regions starting at `base`; returns
    (a, b, next free address).  Shared with tests/test_gpu_chain.py's refusal cases."""
    npix = n * h * w
    cur = [base]

    def take(nbytes):
        p = cur[0]
        cur[0] += (nbytes + 255) // 256 * 256
        return p

    def conv(x, x_ld, cin, co, y, y_ld):
        d = L.ConvDesc()
        d.x, d.y, d.w = x, y, take(co * ((cin + 63) // 64 * 64) * 2)
        d.x_ld, d.y_ld = x_ld, y_ld
        d.n, d.ih, d.iw, d.c, d.kpad, d.cout = n, h, w, cin, (cin + 63) // 64 * 64, co
        d.oh, d.ow, d.sy, d.sx = h, w, 1, 1
        d.th, d.tw, d.dy0, d.dx0, d.ddy, d.ddx = 1, 1, 0, 0, 1, 1
        d.yh, d.yw, d.osy, d.osx, d.ory, d.orx = h, w, 1, 1, 0, 0
        d.dtype, d.out_f32, d.alpha = L.BF16, 0, 0.2
        return d

    x, y, y2 = take(npix * c * 2), take(npix * mid * 2), take(npix * cout * 2)
    a = conv(x, c, c, mid, y, mid)
    b = conv(y, mid, mid, cout, y2, cout)
    a.act, b.act = act, L.ACT_LRELU
    if res:
        a.res, a.res_ld = take(npix * mid * 2), mid
    if bits:
        a.zbits, a.zbits_ld = take(npix * mid // 8), mid // 8
    return a, b, cur[0]


def refusals(base, n, h, w):
    """name -> (a, b) that must not chain"""
    out = {}
    a, b, _ = chain_descs(base, n, h, w, mid=128)
    out["middle width 128"] = (a, b)
    a, b, _ = chain_descs(base, n, h, w, cout=128)
    out["b.cout 128"] = (a, b)
    a, b, _ = chain_descs(base, n, h, w)
    a.beta = 1
    out["beta on a"] = (a, b)
    a, b, _ = chain_descs(base, n, h, w)
    b.beta = 1
    out["beta on b"] = (a, b)
    a, b, _ = chain_descs(base, n, h, w, res=False, bits=False)
    b.out_f32 = 1
    out["fp32 output"] = (a, b)
    a, b, end = chain_descs(base, n, h, w)
    b.x = end  # another buffer of the same shape
    out["b.x is not a.y"] = (a, b)
    a, b, end = chain_descs(base, n, h, w)
    b.res, b.res_ld = end, 64
    out["b with a residual"] = (a, b)
    a, b, end = chain_descs(base, n, h, w, res=False, bits=False)
    a.th = a.tw = 3
    a.dy0 = a.dx0 = -1
    a.kpad = 9 * 64
    a.w = end
    out["a 3x3"] = (a, b)
    return out


def test_refusal_table():
    lib = L.load()
    base = 1 << 32  # plausible, 16-byte aligned, never dereferenced
    a, b, _ = chain_descs(base, 2, 13, 23)
    assert lib.dvie_conv_chain(ctypes.byref(a), ctypes.byref(b)) == 1
    a, b, _ = chain_descs(base, 2, 13, 23, c=32, res=False, act=L.ACT_RELU, bits=False)
    assert lib.dvie_conv_chain(ctypes.byref(a), ctypes.byref(b)) == 1
    for name, (a, b) in refusals(base, 2, 13, 23).items():
        assert lib.dvie_conv_chain(ctypes.byref(a), ctypes.byref(b)) == 0, name
        rc = lib.dvie_conv2d_chain(ctypes.byref(a), ctypes.byref(b), None)
        assert rc == L.DVIE_EINVAL and b"chain" in lib.dvie_last_error(), name
    # an output of one op inside an operand of the other
    a, b, _ = chain_descs(base, 2, 13, 23)
    b.y = a.res + 64
    assert lib.dvie_conv_chain(ctypes.byref(a), ctypes.byref(b)) == 0
    a, b, _ = chain_descs(base, 2, 13, 23)
    b.dact, b.act, b.z, b.z_ld = L.ACT_LRELU, 0, a.y, 256
    assert lib.dvie_conv_chain(ctypes.byref(a), ctypes.byref(b)) == 0
    # a tensor past the 32-bit offsets of one launch
    a, b, _ = chain_descs(base, 64, 1024, 1024)
    assert lib.dvie_conv_chain(ctypes.byref(a), ctypes.byref(b)) == 0
