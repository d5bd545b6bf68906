"""GPU: activation sign bitmaps (include/dvie.h dvie_conv_desc.zbits) through the C ABI.

Producers: a forward 1x1 conv with ReLU / LeakyReLU that is given a bitmap writes
packbits(y_bf16 > 0) next to an unchanged y, and nothing outside the bitmap's region (64-byte
guards and the other channels' bytes of a wider buffer keep their 0xA5 fill).
Consumers: a data gradient with `dact` that is given z + zbits computes exactly what it
computes from z alone; on the dedicated paths z is all NaN in the zbits launch, so a kernel
that still read it would not pass.  Cases per kernel: residual, beta, ReLU / LeakyReLU, ragged
pixel counts, a channel region inside a wider buffer.  dvie_conv_zbits must announce every
dedicated path, and only those (a kernel without one keeps reading z).  head3_bwd_kernel has
no case: it takes act'(h) from the tile of h it stages in LDS for its weight gradient, so it
reads no second stream of z and its descriptor has no bitmap.
Step: the bf16 InterNet step at 2x48x80 with bitmaps and with DVIE_ZBITS=0 gives equal loss
values and equal parameter gradients (torch.equal throughout: the bit comes from the stored
bf16 value, so nothing may differ)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def _packbits(z):
    """[..., C] bf16 -> [..., C / 8] uint8, bit c % 8 of byte c / 8 = (z > 0)"""
    return np.packbits(z.float().cpu().numpy() > 0, axis=-1, bitorder="little")


def _launch(d, what):
    lib = L.load()
    lib.dvie_trace_kernels(1)
    L.check(lib.dvie_conv2d_fwd(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), what)
    torch.cuda.synchronize()
    names = lib.dvie_traced_kernels().decode()
    lib.dvie_trace_kernels(0)
    return names


def _desc(x, wp, y, y_off, n, h, w, c, cout, k):
    d = L.ConvDesc()
    d.x, d.w, d.y = x.data_ptr(), wp.data_ptr(), y.data_ptr() + 2 * y_off
    d.x_ld, d.y_ld = x.shape[-1], y.shape[-1]
    d.n, d.ih, d.iw, d.c, d.kpad, d.cout = n, h, w, c, wp.shape[1], cout
    d.oh, d.ow, d.sy, d.sx = h, w, 1, 1
    d.th, d.tw, d.dy0, d.dx0, d.ddy, d.ddx = k, k, -(k // 2), -(k // 2), 1, 1
    d.yh, d.yw, d.osy, d.osx, d.ory, d.orx = h, w, 1, 1, 0, 0
    d.dtype, d.out_f32, d.alpha = L.BF16, 0, 0.2
    return d


def _weights(g, cout, c, k):
    K = k * k * c
    wt = torch.randn(cout, c, k, k, generator=g) / K ** 0.5
    wp = torch.zeros(cout, (K + 63) // 64 * 64)
    wp[:, :K] = wt.permute(0, 2, 3, 1).reshape(cout, K)
    return wp.to(torch.bfloat16)


# ---------------- producers ----------------
PRODUCERS = [  # kernel, (n, h, w), c, cout, buffer channels, channel offset, act, residual
    ("conv1x1_kernel", (2, 13, 23), 64, 256, 256, 0, L.ACT_RELU, True),    # ragged tile, MFMA-layout stores
    ("conv1x1_kernel", (1, 16, 64), 64, 256, 256, 0, L.ACT_RELU, True),    # full tiles, coalesced epilogue
    ("conv1x1_kernel", (2, 13, 23), 64, 256, 256, 0, L.ACT_LRELU, False),
    ("conv1x1_kernel", (1, 16, 64), 64, 256, 256, 0, L.ACT_LRELU, False),
    ("conv1x1_kernel", (2, 13, 23), 64, 128, 256, 128, L.ACT_LRELU, False),  # a region of a wider buffer
    ("conv1x1_kernel", (1, 16, 64), 64, 128, 256, 128, L.ACT_LRELU, False),
    # the ring kernel: the smallest channel pair of tests/test_gpu_conv1x1_ring.py (192 -> 256), more
    # than 256 tiles of 256 pixels: 257 full pixel tiles, and 258 with a ragged last one
    ("conv1x1_ring_kernel", (1, 257, 256), 192, 256, 256, 0, L.ACT_LRELU, False),
    ("conv1x1_ring_kernel", (1, 259, 255), 192, 256, 256, 0, L.ACT_LRELU, False),
]


@pytest.mark.parametrize("kernel,shape,c,cout,C,c0,act,with_res", PRODUCERS)
def test_forward_writes_the_bitmap(dev, kernel, shape, c, cout, C, c0, act, with_res):
    n, h, w = shape
    npix = n * h * w
    g = torch.Generator().manual_seed(npix + cout + act)
    x = torch.randn(n, h, w, c, generator=g)
    x.view(npix, c)[::5] = 0  # whole pixels of zeros: exact zeros in the output
    x = x.to(torch.bfloat16).to(dev)
    wp = _weights(g, cout, c, 1).to(dev)
    res = None
    if with_res:
        res = torch.randn(n, h, w, cout, generator=g)
        res.view(npix, cout)[::5] = 0
        res = res.to(torch.bfloat16).to(dev)
    bias = None
    if act == L.ACT_LRELU:  # a denormal negative bias: the zero pixels give -0.0 after the slope
        bias = torch.zeros(cout)
        bias[::3] = -1e-40
        bias = bias.to(dev)
    outs = []
    for with_bits in (False, True):
        y = torch.full((n, h, w, C), 7.0, dtype=torch.bfloat16, device=dev)
        bm = torch.full((GUARD + npix * C // 8 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        d = _desc(x, wp, y, c0, n, h, w, c, cout, 1)
        d.act = act
        if res is not None:
            d.res, d.res_ld = res.data_ptr(), cout
        if bias is not None:
            d.bias = bias.data_ptr()
        if with_bits:
            d.zbits, d.zbits_ld = bm.data_ptr() + GUARD + c0 // 8, C // 8
            assert L.load().dvie_conv_zbits(ctypes.byref(d)) == (2 if kernel == "conv1x1_ring_kernel" else 1)
        names = _launch(d, "producer")
        assert kernel in names, names
        outs.append((y.cpu(), bm.cpu().numpy()))
    (y0, bm0), (y1, bm1) = outs
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
    assert (bm0 == 0xA5).all()
    want = np.full((npix, C // 8), 0xA5, dtype=np.uint8)
    yr = y1[..., c0:c0 + cout].reshape(npix, cout)
    bits = _packbits(yr)
    want[:, c0 // 8:(c0 + cout) // 8] = bits
    assert (bm1[:GUARD] == 0xA5).all() and (bm1[-GUARD:] == 0xA5).all()
    got = bm1[GUARD:-GUARD].reshape(npix, C // 8)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    frac = float((yr.float() > 0).float().mean())
    print(f"{kernel} {shape} {c}->{cout}@{c0}/{C} act {act}: {frac:.2f} positive ({names})")
    assert 0.25 < frac < 0.75 and bits.any() and not (bits == 0xFF).all()
    raw = yr.contiguous().view(torch.int16)
    assert bool((raw == 0).any() | (raw == -32768).any()), "no exact zero in the output"
    if act == L.ACT_LRELU:
        assert bool((raw == -32768).any()), "no -0.0 in the output"
        assert bool((yr.float() < 0).any())


# ---------------- consumers ----------------
P_RAG, P_FULL = (2, 13, 23), (1, 16, 64)
H8_SHAPE = (4, 60, 450)  # 4 x 8 x 8 eight-row tiles of 64 columns (ragged both ways): >= 224
CONSUMERS = [  # kernel, dedicated path, (n, h, w), c, cout, buffer channels, offset, k, dact, res, beta
    ("conv1x1_kernel", True, P_RAG, 64, 256, 256, 0, 1, L.ACT_LRELU, False, 0),
    ("conv1x1_kernel", True, P_RAG, 64, 256, 256, 0, 1, L.ACT_RELU, True, 0),   # row-coalesced residual
    ("conv1x1_kernel", True, P_FULL, 64, 256, 256, 0, 1, L.ACT_RELU, True, 0),
    ("conv1x1_kernel", True, P_FULL, 64, 256, 256, 0, 1, L.ACT_LRELU, False, 1),
    ("conv1x1_kernel", True, P_FULL, 64, 256, 256, 0, 1, L.ACT_LRELU, True, 1),
    ("conv1x1_kernel", True, P_RAG, 64, 256, 512, 256, 1, L.ACT_RELU, True, 1),  # a region of a wider buffer
    ("conv1x1_kernel", True, P_FULL, 64, 256, 512, 256, 1, L.ACT_LRELU, False, 0),
    ("conv_h8_kernel", True, H8_SHAPE, 64, 128, 128, 0, 3, L.ACT_LRELU, False, 0),
    ("conv_h8_kernel", True, H8_SHAPE, 64, 128, 128, 0, 3, L.ACT_RELU, True, 1),
    ("conv_h8_kernel", True, H8_SHAPE, 64, 128, 256, 128, 3, L.ACT_RELU, False, 1),
    ("conv_h8_kernel", True, H8_SHAPE, 64, 128, 256, 128, 3, L.ACT_LRELU, True, 0),
    # the dense-K kernel (c <= 24), ragged tiles; 96 and 64 output channels (a partial / a whole
    # 64-channel block per workgroup column)
    ("conv_nk_kernel", True, (1, 9, 33), 24, 96, 96, 0, 3, L.ACT_LRELU, False, 0),
    ("conv_nk_kernel", True, (1, 9, 33), 24, 96, 96, 0, 3, L.ACT_RELU, True, 1),
    ("conv_nk_kernel", True, (2, 13, 70), 16, 64, 128, 64, 3, L.ACT_LRELU, True, 0),
    ("conv_nk_kernel", True, (2, 13, 70), 8, 64, 128, 64, 3, L.ACT_RELU, False, 1),
    # no dedicated path (several K-steps): the kernel reads z, the descriptor's bitmap is ignored
    ("conv1x1_kernel", False, P_RAG, 128, 256, 256, 0, 1, L.ACT_LRELU, True, 1),
    ("conv1x1_kernel", False, P_RAG, 128, 128, 256, 128, 1, L.ACT_RELU, False, 0),
]


@pytest.mark.parametrize("kernel,dedicated,shape,c,cout,C,c0,k,dact,with_res,beta", CONSUMERS)
def test_data_gradient_reads_the_bitmap(dev, kernel, dedicated, shape, c, cout, C, c0, k, dact, with_res, beta):
    n, h, w = shape
    npix = n * h * w
    g = torch.Generator().manual_seed(npix + cout + 7 * dact + c0)
    x = torch.randn(n, h, w, c, generator=g).to(torch.bfloat16).to(dev)
    wp = _weights(g, cout, c, k).to(dev)
    z = torch.randn(n, h, w, C, generator=g)
    zf = z.view(-1)
    zf[::7] = 0.0
    zf[3::11] = -0.0
    z = z.to(torch.bfloat16)
    bits = torch.from_numpy(_packbits(z))  # [n, h, w, C / 8], from z itself, not from a producer
    res = torch.randn(n, h, w, cout, generator=g).to(torch.bfloat16).to(dev) if with_res else None
    y_old = torch.randn(n, h, w, C, generator=g).to(torch.bfloat16)
    outs = []
    for with_bits in (False, True):
        y = y_old.clone().to(dev)
        # a dedicated path must not read z: poisoned (a copy; the reference launch has z intact)
        zd = torch.full_like(z, float("nan")).to(dev) if with_bits and dedicated else z.to(dev)
        bm = bits.to(dev)
        d = _desc(x, wp, y, c0, n, h, w, c, cout, k)
        d.dact, d.beta = dact, beta
        d.z, d.z_ld = zd.data_ptr() + 2 * c0, C
        if res is not None:
            d.res, d.res_ld = res.data_ptr(), cout
        if with_bits:
            d.zbits, d.zbits_ld = bm.data_ptr() + c0 // 8, C // 8
            assert L.load().dvie_conv_zbits(ctypes.byref(d)) == int(dedicated)
        names = _launch(d, "consumer")
        assert kernel in names, names
        outs.append(y.cpu())
        assert torch.equal(bm.cpu(), bits)
    a, b = (o.view(torch.int16) for o in outs)
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} elements differ ({names})"
    assert bool(torch.isfinite(outs[1].float()).all())
    assert not torch.equal(outs[0][..., c0:c0 + cout], y_old[..., c0:c0 + cout])
    print(f"{kernel} {shape} {c}->{cout}@{c0}/{C} k{k} dact {dact} res {with_res} beta {beta}: equal ({names})")


# ---------------- the training step ----------------
def _step(dev, setattr_):
    from bench import make_batch
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
    plans = []
    compile_ = E.Graph.compile

    def compile_and_keep(self, *a, **k):
        plans.append(compile_(self, *a, **k))
        return plans[-1]

    setattr_(E.Graph, "compile", compile_and_keep)
    trainer = InterTrainer(args)
    ld = trainer.forward_backward(make_batch(batch, H, W, dev, 0))
    torch.cuda.synchronize()
    setattr_(E.Graph, "compile", compile_)
    hr = trainer.model.module.coarse_model
    grads = {name: p.grad.detach().clone() for name, p in hr.named_parameters() if p.grad is not None}
    return {k: v.clone() for k, v in ld.items()}, grads, sum(len(q.zbits) for q in plans), len(plans)


def test_step_is_equal_with_and_without_bitmaps(dev, monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    monkeypatch.setenv("DVIE_PRECISION", "bf16")
    monkeypatch.setenv("DVIE_ZBITS", "1")
    ld1, g1, nb1, np1 = _step(dev, monkeypatch.setattr)
    monkeypatch.setenv("DVIE_ZBITS", "0")
    ld0, g0, nb0, np0 = _step(dev, monkeypatch.setattr)
    print(f"bitmaps: {nb1} in {np1} plan(s) with DVIE_ZBITS=1, {nb0} in {np0} with 0; {len(g1)} gradients")
    assert nb0 == 0 and nb1 > 0 and np1 == np0 > 0
    assert ld1.keys() == ld0.keys() and len(g1) > 50 and g1.keys() == g0.keys()
    for k in ld1:
        assert torch.equal(ld1[k], ld0[k]), (k, ld1[k], ld0[k])
    for k in g1:
        assert torch.equal(g1[k], g0[k]), k
