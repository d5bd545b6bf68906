"""GPU: chained 1x1 launches (include/dvie.h dvie_conv_chain, dvie_conv2d_chain,
dvie_ops_chain_pairs; csrc/conv_chain.hip) through the C ABI.

A pair (a: c <= 64 -> 256 channels, b: 256 -> 64 channels reading a's output) runs three ways:
(a) one dvie_run_ops call of the 2-op array, (b) two calls of one op each, (c) dvie_conv2d_chain.
y, the bitmap and the second output, each 7.0 / 0xA5-filled inside 64-byte guards, must be equal
byte for byte across the three, guards and the other channels of a wider buffer included; the
launch trace shows conv1x1_chain_kernel alone for (a) and (c) and the two single kernels for
(b).  (b) is also held to an fp64 evaluation within plan_ref.BARS["act"] (relative L2), so the
equality does not compare one error with itself.

The built kernel walks 64-pixel tiles with at most 256 persistent workgroups.  Shapes: 1x5x7
(35 pixels, less than a tile), 2x13x23 (598 = 9 tiles + 22), 2x97x199 (38,606 = 603 tiles + 14:
workgroups run two or three tiles, the last one ragged).
Epilogues: forward -- bias + residual + LeakyReLU + bitmap, the same with ReLU, without the
residual, without the bitmap, b with bias + LeakyReLU; backward -- residual + derivative from
the bitmap (z all NaN: a launch that read it would not pass), derivative from z without a
bitmap, b with the derivative from its 64-channel z.  Also c = 32 (channel padding inside the
K-step) and both outputs as channel regions of wider buffers.
Refusals (middle width 128, b.cout 128, beta, fp32 output, b.x != a.y, b with a residual, a 3x3
a) run unfused with (b)'s bytes.  Look-ahead: a weight gradient on lane 1 between the two is
skipped over and runs after the chained launch; one that reads b's output blocks the pairing.
Step: the bf16 InterNet step at 2x48x80 with DVIE_CHAIN=0 and 1, each in a fresh process: equal
losses and gradients; one chained step launches conv1x1_chain_kernel 5 times (3 forward pairs,
2 backward: tests/test_chain_cpu.py says why not 3)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import plan_ref
from deep_video_interpolation_extrapolation_amd import _lib as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SMALL, RAGGED, MULTI = (1, 5, 7), (2, 13, 23), (2, 97, 199)


@pytest.fixture(autouse=True)
def _chain_on(monkeypatch):
    monkeypatch.setenv("DVIE_CHAIN", "1")


class Buf:
    """a 7.0- (bf16 / fp32) or 0xA5-filled (uint8) tensor inside 64-byte guards"""

    def __init__(self, dev, numel, dtype):
        self.dtype, self.numel = dtype, numel
        self.g = GUARD // torch.empty(0, dtype=dtype).element_size()
        self.full = torch.empty(numel + 2 * self.g, dtype=dtype, device=dev)
        self.reset()

    def reset(self):
        if self.dtype == torch.uint8:
            self.full.fill_(0xA5)
        else:
            self.full.fill_(7.0)

    @property
    def ptr(self):
        return self.full.data_ptr() + GUARD

    @property
    def data(self):
        return self.full[self.g:self.g + self.numel]

    def guards_intact(self):
        fill = 0xA5 if self.dtype == torch.uint8 else 7.0
        return bool((self.full[:self.g] == fill).all()) and bool((self.full[-self.g:] == fill).all())

    def raw(self):
        return self.full.view(torch.uint8).clone()


def _weights(g, cout, c, k=1):
    K = k * k * c
    wt = torch.randn(cout, c, k, k, generator=g) / K ** 0.5
    wp = torch.zeros(cout, (K + 63) // 64 * 64)
    wp[:, :K] = wt.permute(0, 2, 3, 1).reshape(cout, K)
    return wp.to(torch.bfloat16)


def _desc(x_ptr, x_ld, wp, y_ptr, y_ld, n, h, w, c, cout, k=1):
    d = L.ConvDesc()
    d.x, d.w, d.y = x_ptr, wp.data_ptr(), y_ptr
    d.x_ld, d.y_ld = x_ld, y_ld
    d.n, d.ih, d.iw, d.c, d.kpad, d.cout = n, h, w, c, wp.shape[1], cout
    d.oh, d.ow, d.sy, d.sx = h, w, 1, 1
    d.th, d.tw, d.dy0, d.dx0, d.ddy, d.ddx = k, k, -(k // 2), -(k // 2), 1, 1
    d.yh, d.yw, d.osy, d.osx, d.ory, d.orx = h, w, 1, 1, 0, 0
    d.dtype, d.out_f32, d.alpha = L.BF16, 0, 0.2
    return d


class Pair:
    """The two descriptors and their tensors.  mode "fwd": a = bias + res + act (+ bitmap), b =
    bias + LeakyReLU; mode "bwd": a = res + derivative (bitmap or z), b = derivative from z."""

    def __init__(self, dev, shape, mode, act=L.ACT_LRELU, res=True, bits=True, c=64, mid=256, cout=64,
                 wide=False, k=1, b_f32=False):
        n, h, w = shape
        self.shape, self.mode, self.act, self.mid, self.cout, self.c = shape, mode, act, mid, cout, c
        npix = self.npix = n * h * w
        g = torch.Generator().manual_seed(npix + 3 * act + c + mid + (7 if wide else 0))
        self.Cy, self.c0 = (mid + 256, 128) if wide else (mid, 0)    # a's output region
        self.Cy2, self.c02 = (cout + 64, 32) if wide else (cout, 0)  # b's output region
        x = torch.randn(npix, c, generator=g)
        x[::5] = 0
        self.x = x.to(torch.bfloat16).to(dev)
        self.w1, self.w2 = _weights(g, mid, c, k).to(dev), _weights(g, cout, mid).to(dev)
        self.y = Buf(dev, npix * self.Cy, torch.bfloat16)
        self.y2 = Buf(dev, npix * self.Cy2, torch.float32 if b_f32 else torch.bfloat16)
        self.bm = Buf(dev, npix * self.Cy // 8, torch.uint8)
        a = _desc(self.x.data_ptr(), c, self.w1, self.y.ptr + 2 * self.c0, self.Cy, n, h, w, c, mid, k)
        b = _desc(self.y.ptr + 2 * self.c0, self.Cy, self.w2, self.y2.ptr + (4 if b_f32 else 2) * self.c02, self.Cy2,
                  n, h, w, mid, cout)
        b.out_f32 = int(b_f32)
        self.res = self.bias1 = self.bias2 = self.z1 = self.z1_dev = self.z2 = None
        if res:
            r = torch.randn(npix, mid, generator=g)
            r[::5] = 0
            self.res = r.to(torch.bfloat16).to(dev)
            a.res, a.res_ld = self.res.data_ptr(), mid
        if mode == "fwd":
            self.bias1 = torch.randn(mid, generator=g).mul_(0.1)
            self.bias1[::3] = -1e-40  # with the zero pixels: -0.0 after the slope
            self.bias1 = self.bias1.to(dev)
            self.bias2 = torch.randn(cout, generator=g).mul_(0.1).to(dev)
            a.bias, b.bias = self.bias1.data_ptr(), self.bias2.data_ptr()
            a.act, b.act = act, L.ACT_LRELU
            if bits:
                a.zbits, a.zbits_ld = self.bm.ptr + self.c0 // 8, self.Cy // 8
        else:
            z1 = torch.randn(npix, self.Cy, generator=g)
            z1.view(-1)[::7] = 0.0
            z1.view(-1)[3::11] = -0.0
            self.z1 = z1.to(torch.bfloat16).to(dev)
            z2 = torch.randn(npix, cout, generator=g)
            z2.view(-1)[::7] = 0.0
            self.z2 = z2.to(torch.bfloat16).to(dev)
            a.dact, b.dact = act, L.ACT_LRELU
            b.z, b.z_ld = self.z2.data_ptr(), cout
            self.z1_dev = self.z1
            if bits:  # the bitmap of z1; z itself poisoned
                import numpy as np
                pk = np.packbits(self.z1.float().cpu().numpy() > 0, axis=-1, bitorder="little")
                self.bm.data.copy_(torch.from_numpy(pk).reshape(-1).to(dev))
                self.bm_fill = self.bm.full.clone()
                a.zbits, a.zbits_ld = self.bm.ptr + self.c0 // 8, self.Cy // 8
                self.z1_dev = torch.full_like(self.z1, float("nan"))
            a.z, a.z_ld = self.z1_dev.data_ptr() + 2 * self.c0, self.Cy
        self.a, self.b = a, b
        self.reads_bits = mode == "bwd" and bits

    def reset(self):
        self.y.reset()
        self.y2.reset()
        if self.reads_bits:
            self.bm.full.copy_(self.bm_fill)
        else:
            self.bm.reset()

    def ops(self, between=()):
        descs = [("conv", self.a, 0)] + list(between) + [("conv", self.b, 0)]
        arr = (L.Op * len(descs))()
        for o, (kind, d, lane) in zip(arr, descs):
            o.lane = lane
            if kind == "conv":
                o.kind, o.u.conv = L.OP_CONV, d
            else:
                o.kind, o.u.wgrad = L.OP_WGRAD, d
        return arr

    def snapshot(self):
        torch.cuda.synchronize()
        assert self.y.guards_intact() and self.y2.guards_intact() and self.bm.guards_intact()
        return self.y.raw(), self.bm.raw(), self.y2.raw()

    def chains(self):
        return L.load().dvie_conv_chain(ctypes.byref(self.a), ctypes.byref(self.b))

    def reference_errors(self):
        """relative L2 of the stored y and second output against fp64 on the same operands"""
        f = torch.float64
        c, mid = self.c, self.mid

        def act(v, kind):
            return torch.where(v > 0, v, v * (0.2 if kind == L.ACT_LRELU else 0.0))

        def dact(z, kind):
            one = torch.ones((), dtype=f, device=z.device)
            return torch.where(z > 0, one, one * (0.2 if kind == L.ACT_LRELU else 0.0))

        v = self.x.to(f) @ self.w1[:, :c].to(f).T
        if self.bias1 is not None:
            v = v + self.bias1.to(f)
        if self.res is not None:
            v = v + self.res.to(f)
        if self.mode == "fwd":
            v = act(v, self.act)
        else:
            v = v * dact(self.z1[:, self.c0:self.c0 + mid].to(f), self.act)
        y = self.y.data.view(self.npix, self.Cy)[:, self.c0:self.c0 + mid]
        e1 = plan_ref.rel_l2(y, v)
        v2 = y.to(f) @ self.w2[:, :mid].to(f).T  # b reads the stored bf16 y
        if self.bias2 is not None:
            v2 = v2 + self.bias2.to(f)
        v2 = act(v2, L.ACT_LRELU) if self.mode == "fwd" else v2 * dact(self.z2.to(f), L.ACT_LRELU)
        y2 = self.y2.data.view(self.npix, self.Cy2)[:, self.c02:self.c02 + self.cout]
        return e1, plan_ref.rel_l2(y2, v2)


def _traced(fn):
    lib = L.load()
    lib.dvie_trace_kernels(1)
    fn()
    torch.cuda.synchronize()
    names = lib.dvie_traced_kernels().decode()
    lib.dvie_trace_kernels(0)
    return [k for k in names.split(";") if k]


def _run_ops(arr, start, n):
    lib = L.load()
    base = ctypes.addressof(arr) + start * ctypes.sizeof(L.Op)
    L.check(lib.dvie_run_ops(base, n, L.stream_ptr()), "run_ops")


def _three_ways(p, expect_chain=True):
    lib = L.load()
    arr = p.ops()
    p.reset()
    k_a = _traced(lambda: _run_ops(arr, 0, 2))
    s_a = p.snapshot()
    p.reset()
    k_b = _traced(lambda: (_run_ops(arr, 0, 1), _run_ops(arr, 1, 1)))
    s_b = p.snapshot()
    errs = p.reference_errors() if not p.b.out_f32 and p.a.th == 1 else None
    assert len(k_b) == 2 and not any("chain" in k for k in k_b), k_b
    for name, u, v in zip(("y", "bitmap", "second output"), s_a, s_b):
        assert torch.equal(u, v), f"run_ops pair vs single ops: {name}: {int((u != v).sum())} bytes differ ({k_a})"
    if expect_chain:
        assert p.chains() == 1
        assert len(k_a) == 1 and "conv1x1_chain_kernel" in k_a[0], k_a
        assert all(k.startswith(("void dvie::conv1x1_", "dvie::conv1x1_", "conv1x1_")) for k in k_b), k_b
        p.reset()
        k_c = _traced(lambda: L.check(lib.dvie_conv2d_chain(ctypes.byref(p.a), ctypes.byref(p.b), L.stream_ptr()), "chain"))
        s_c = p.snapshot()
        assert len(k_c) == 1 and "conv1x1_chain_kernel" in k_c[0], k_c
        for name, u, v in zip(("y", "bitmap", "second output"), s_c, s_b):
            assert torch.equal(u, v), f"dvie_conv2d_chain vs single ops: {name}: {int((u != v).sum())} bytes differ"
    else:
        assert p.chains() == 0
        assert k_a == k_b, (k_a, k_b)
        rc = lib.dvie_conv2d_chain(ctypes.byref(p.a), ctypes.byref(p.b), L.stream_ptr())
        assert rc == L.DVIE_EINVAL
    return errs, k_a, k_b


EPILOGUES = {  # mode, activation, residual, bitmap
    "fwd-lrelu-res-bits": ("fwd", L.ACT_LRELU, True, True),
    "fwd-relu-res-bits": ("fwd", L.ACT_RELU, True, True),
    "fwd-lrelu-bits": ("fwd", L.ACT_LRELU, False, True),
    "fwd-lrelu-res": ("fwd", L.ACT_LRELU, True, False),
    "bwd-res-bits": ("bwd", L.ACT_RELU, True, True),
    "bwd-res-z": ("bwd", L.ACT_LRELU, True, False),
    "bwd-z": ("bwd", L.ACT_LRELU, False, False),
}


@pytest.mark.parametrize("shape", [SMALL, RAGGED, MULTI], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("epi", list(EPILOGUES))
def test_chain_equals_two_launches(dev, shape, epi):
    mode, act, res, bits = EPILOGUES[epi]
    p = Pair(dev, shape, mode, act=act, res=res, bits=bits)
    (e1, e2), k_a, k_b = _three_ways(p)
    print(f"{epi} {shape}: rel L2 vs fp64 y {e1:.2e}, second output {e2:.2e} (bar {plan_ref.BARS['act']}); {k_a[0][:60]}")
    assert e1 <= plan_ref.BARS["act"] and e2 <= plan_ref.BARS["act"], (e1, e2)
    if mode == "fwd" and bits:  # the bitmap is packbits(y > 0) and not the fill
        import numpy as np
        y = p.y.data.view(p.npix, p.Cy)
        want = np.packbits(y.float().cpu().numpy() > 0, axis=-1, bitorder="little")
        assert np.array_equal(p.bm.data.cpu().numpy().reshape(p.npix, -1), want)
    if p.reads_bits:
        assert torch.equal(p.bm.full, p.bm_fill) and bool(torch.isfinite(p.y.data.float()).all())


@pytest.mark.parametrize("shape", [RAGGED, MULTI], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("epi", ["fwd-relu-res-bits", "bwd-res-bits"])
def test_chain_channel_padding_and_wide_buffers(dev, shape, epi):
    mode, act, res, bits = EPILOGUES[epi]
    for kw in (dict(c=32), dict(wide=True), dict(c=8, wide=True)):
        p = Pair(dev, shape, mode, act=act, res=res, bits=bits, **kw)
        (e1, e2), k_a, _ = _three_ways(p)
        print(f"{epi} {shape} {kw}: rel L2 vs fp64 y {e1:.2e}, second output {e2:.2e}")
        assert e1 <= plan_ref.BARS["act"] and e2 <= plan_ref.BARS["act"], (kw, e1, e2)
        if kw.get("wide"):  # the other channels of both buffers keep their fill
            y = p.y.data.view(p.npix, p.Cy)
            y2 = p.y2.data.view(p.npix, p.Cy2)
            assert bool((y[:, :p.c0] == 7.0).all()) and bool((y[:, p.c0 + p.mid:] == 7.0).all())
            assert bool((y2[:, :p.c02] == 7.0).all()) and bool((y2[:, p.c02 + p.cout:] == 7.0).all())


def _refusal(dev, name):
    kw = dict(shape=RAGGED, mode="fwd")
    if name == "middle width 128":
        return Pair(dev, mid=128, **kw)
    if name == "b.cout 128":
        return Pair(dev, cout=128, **kw)
    if name == "fp32 output":
        return Pair(dev, b_f32=True, **kw)
    if name == "a 3x3":
        return Pair(dev, k=3, res=False, bits=False, **kw)
    p = Pair(dev, **kw)
    if name == "beta":
        p.b.beta = 1
    elif name == "b.x is not a.y":
        p.other = torch.randn(p.npix, 256, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).to(dev)
        p.b.x = p.other.data_ptr()
        p.b.x_ld = 256
    elif name == "b with a residual":
        p.res2 = torch.randn(p.npix, 64, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16).to(dev)
        p.b.res, p.b.res_ld = p.res2.data_ptr(), 64
    return p


@pytest.mark.parametrize("name", ["middle width 128", "b.cout 128", "beta", "fp32 output", "b.x is not a.y",
                                  "b with a residual", "a 3x3"])
def test_refused_pairs_run_unfused(dev, name):
    p = _refusal(dev, name)
    _, k_a, k_b = _three_ways(p, expect_chain=False)
    print(f"{name}: {k_a}")


def _wgrad(dev, p, g_ptr, g_ld, cout):
    """weight gradient of a 1x1 conv over p's pixels: g (cout channels) x p.x (64 channels)"""
    lib = L.load()
    n, h, w = p.shape
    d = L.WgradDesc()
    d.g, d.x = g_ptr, p.x.data_ptr()
    d.g_ld, d.x_ld = g_ld, p.c
    d.n, d.oh, d.ow, d.cout = n, h, w, cout
    d.ih, d.iw, d.c, d.sy, d.sx = h, w, p.c, 1, 1
    d.th, d.tw, d.dy0, d.dx0, d.ddy, d.ddx = 1, 1, 0, 0, 1, 1
    d.dtype = L.BF16
    hint = lib.dvie_wgrad_splits_hint(ctypes.byref(d))
    d.splits = hint if hint > 0 else 4
    ws = torch.full((lib.dvie_wgrad_slabs(ctypes.byref(d)) * cout * p.c,), float("nan"), device=dev)
    d.ws = ws.data_ptr()
    return d, ws


def test_look_ahead_over_a_weight_gradient(dev):
    p = Pair(dev, RAGGED, "fwd")
    d, ws = _wgrad(dev, p, p.a.y, p.Cy, 256)  # reads a's output and the 64-channel x
    arr = p.ops(between=[("wgrad", d, 1)])
    partner = (ctypes.c_int * 3)()
    assert L.load().dvie_ops_chain_pairs(arr, 3, partner) == 1 and list(partner) == [2, -1, 0]
    p.reset()
    k_a = _traced(lambda: _run_ops(arr, 0, 3))
    s_a, ws_a = p.snapshot(), ws.clone()
    assert "conv1x1_chain_kernel" in k_a[0] and len(k_a) >= 2 and not any("conv1x1" in k for k in k_a[1:]), k_a
    p.reset()
    ws.fill_(float("nan"))
    k_b = _traced(lambda: [_run_ops(arr, i, 1) for i in range(3)])
    s_b = p.snapshot()
    assert not any("chain" in k for k in k_b), k_b
    for u, v in zip(s_a, s_b):
        assert torch.equal(u, v)
    assert torch.equal(ws_a.view(torch.int32), ws.view(torch.int32)) and bool(torch.isfinite(ws).all())


def test_look_ahead_stops_at_a_reader_of_the_second_output(dev):
    p = Pair(dev, RAGGED, "fwd")
    p.y2.data.copy_(torch.randn(p.npix * 64, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16))
    d, ws = _wgrad(dev, p, p.b.y, 64, 64)  # reads b's output buffer
    arr = p.ops(between=[("wgrad", d, 1)])
    partner = (ctypes.c_int * 3)()
    assert L.load().dvie_ops_chain_pairs(arr, 3, partner) == 0 and list(partner) == [-1, -1, -1]
    k_a = _traced(lambda: _run_ops(arr, 0, 3))
    assert not any("chain" in k for k in k_a) and sum("conv1x1_" in k for k in k_a) == 2, k_a


# ---------------- the training step, each setting in a fresh process ----------------
_STEP = r"""
import json, sys, torch
sys.path.insert(0, sys.argv[1])
from bench import make_batch
from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import engine as E
from deep_video_interpolation_extrapolation_amd.options import default_args
from deep_video_interpolation_extrapolation_amd.runners.InterTrainer import InterTrainer

class _Log:
    def info(self, msg):
        pass

batch, H, W = 2, 48, 80
args = default_args("INTER", syn_type="inter", interval=5, mode="xs2xs", vid_length=1, train_coarse=True,
                    batch_size=batch, input_h=H, input_w=W, precision="bf16", synthetic=batch, num_workers=0,
                    split="train", rank=0, gpus=1)
args.logger = _Log()
torch.manual_seed(args.seed)
dev = torch.device("cuda:0")
trainer = InterTrainer(args)
lib = L.load()
# the plans' op lists run on two host threads (forward: this one, backward: autograd's), and the
# launch trace is per thread: record around every dvie_run_ops batch, on the thread that runs it
traced = []
plan_run = E.Plan._run

def traced_run(self, *a, **k):
    lib.dvie_trace_kernels(1)
    try:
        return plan_run(self, *a, **k)
    finally:
        traced.append(lib.dvie_traced_kernels().decode())
        lib.dvie_trace_kernels(0)

E.Plan._run = traced_run
ld = trainer.forward_backward(make_batch(batch, H, W, dev, 0))
torch.cuda.synchronize()
E.Plan._run = plan_run
names = ";".join(traced)
hr = trainer.model.module.coarse_model
out = {"loss": {k: v.detach().float().cpu() for k, v in ld.items()},
       "grad": {n: p.grad.detach().cpu() for n, p in hr.named_parameters() if p.grad is not None},
       "chain": names.count("conv1x1_chain_kernel"), "launches": len([k for k in names.split(";") if k])}
torch.save(out, sys.argv[2])
"""


def _step(tmp_path, chain):
    script, out = tmp_path / "step.py", tmp_path / f"step{chain}.pt"
    script.write_text(_STEP)
    env = dict(os.environ, DVIE_CHAIN=str(chain), DVIE_PRECISION="bf16", DVIE_ZBITS="1")
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return torch.load(out)


def test_step_is_equal_with_and_without_the_chain(dev, tmp_path):
    on, off = _step(tmp_path, 1), _step(tmp_path, 0)
    print(f"chained step: {on['chain']} chained launches of {on['launches']}; unchained: {off['chain']} of {off['launches']}")
    assert off["chain"] == 0
    # 3 forward pairs and the 2 backward pairs the plan's op order allows (tests/test_chain_cpu.py)
    assert on["chain"] == 5 and on["launches"] == off["launches"] - 5
    assert on["loss"].keys() == off["loss"].keys() and len(on["grad"]) > 50 and on["grad"].keys() == off["grad"].keys()
    for k in on["loss"]:
        assert torch.equal(on["loss"][k], off["loss"][k]), (k, on["loss"][k], off["loss"][k])
    for k in on["grad"]:
        assert torch.equal(on["grad"][k], off["grad"][k]), k
