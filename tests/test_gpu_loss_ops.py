"""Op-level parity of the loss and metric reductions -- the nine kinds of dvie_loss (L1, GDL, SSIM,
MSE, CE, L1NHWC, COSNHWC, IOU, ARGMAX_IOU), dvie_sum_f32, dvie_reparam_fwd / dvie_reparam_bwd --
called through ctypes with every descriptor field set here, against the fp64 references of
tests/loss_ref.py.

Comparison: |got - ref| <= tolerance, elementwise, with the bounds of loss_ref (derived from the
kernels' roundings or, for SSIM, measured on the fp32 CPU oracle; never from a kernel's output).
Every test prints `RATIO <output>: max error / tolerance`; DESIGN.md ("Loss-op tests") records
them.

Memory: every buffer a kernel writes (grad, out, partial, ws, z, gmu, glogvar) lives inside a
0xA5-filled allocation with a 64 KiB guard band on both sides (test_gpu_gan_ops.Guarded) and is
sized by the library's own queries.  A buffer the kernel is to overwrite starts as NaN, so an
element it skips fails the comparison (or the all-finite check of partial and ws); a buffer it
is to accumulate into starts with known values.  The guards are compared after every call.
"""
import ctypes
import functools
import math

import pytest
import torch

import loss_ref as R
from deep_video_interpolation_extrapolation_amd import _lib as L
from test_gpu_gan_ops import Guarded, call, close

pytestmark = pytest.mark.gpu

EPS = R.EPS
NAN = float("nan")
RAGGED = (2, 3, 17, 23)
KIND = {"l1": L.LOSS_L1, "gdl": L.LOSS_GDL, "ssim": L.LOSS_SSIM}


def place(t, how, dev):
    """device tensor with t's values: 'dense', 'cl' (NCHW view of NHWC memory) or 'in' (the
    interior slice of a larger PAD_VALUE-filled tensor)"""
    if how == "in":
        _, big = R.interior(t)
        b, c, h, w = t.shape
        return big.to(dev)[:, 1:1 + c, 2:2 + h, 3:3 + w]
    if how == "cl":
        return R.channels_last(t.to(dev))
    return t.to(dev).contiguous()


def nan_buf(G, shape, dtype, name):
    t = G.alloc(shape, dtype, name)
    t.fill_(NAN)
    return t


def desc4(kind, a, b, sa, sb, dims, dtype=L.F32, weight=1.0, out_scale=1.0):
    d = L.LossDesc()
    d.kind, d.a, d.b, d.dtype = kind, a, b, dtype
    d.a_sn, d.a_sc, d.a_sh, d.a_sw = sa
    d.b_sn, d.b_sc, d.b_sh, d.b_sw = sb
    d.bsz, d.ch, d.h, d.w = dims
    d.weight, d.out_scale = weight, out_scale
    return d


def launch(dev, d, nout=1, out_prior=None, grad_shape=None, grad_prior=None, use_ws=True):
    """allocate out / partial / grad / ws for the descriptor (guarded, NaN or the priors), call
    dvie_loss, check the guards -> (out, grad or None, partial count)"""
    lib = L.load()
    G = Guarded(dev)
    npart = lib.dvie_loss_partial_count(ctypes.byref(d))
    assert npart >= 1
    partial = nan_buf(G, (npart,), torch.float64, "partial")
    out = G.put(out_prior, "out") if out_prior is not None else nan_buf(G, (nout,), torch.float32, "out")
    d.partial, d.out, d.out_acc = partial.data_ptr(), out.data_ptr(), int(out_prior is not None)
    grad = ws = None
    if grad_shape is not None:
        grad = G.put(grad_prior, "grad") if grad_prior is not None else nan_buf(G, grad_shape, torch.float32, "grad")
        d.grad, d.beta = grad.data_ptr(), int(grad_prior is not None)
        nws = lib.dvie_loss_ws_floats(ctypes.byref(d))
        assert nws == (3 * math.prod(grad_shape) if d.kind == L.LOSS_SSIM else 0)
        if nws and use_ws:
            ws = nan_buf(G, (nws,), torch.float32, "ws")
            d.ws = ws.data_ptr()
    call(lib.dvie_loss, ctypes.byref(d), L.stream_ptr(dev))
    G.check()
    assert bool(torch.isfinite(partial).all()), "a partial sum was not written"
    if ws is not None:
        assert bool(torch.isfinite(ws).all()), "an adjoint map element was not written"
    return out.cpu(), (grad.cpu() if grad is not None else None), npart


# ---------------- L1, GDL, SSIM ----------------
@functools.lru_cache(maxsize=None)
def pixel_ref(kind, builder, shape, weight):
    """(a, b, value, bound of the value before the store | None, SSIM value tolerance | None,
    gradient, gradient tolerance), computed once per case and shared"""
    if builder == "grid":
        a, b = R.grid_pair(shape, 100 + sum(shape))
    elif builder == "degenerate":
        a, b = R.ssim_near_degenerate(shape)
    else:
        a, b = R.ssim_flat(shape)
    if kind == "ssim":
        t = R.ssim_tolerance(a, b, weight)
        return a, b, t.value, None, t.tol_value, t.grad, t.tol_grad
    r = (R.l1 if kind == "l1" else R.gdl)(a, b, weight)
    return a, b, r.value, r.bound, None, r.grad, r.tol_grad


def run_pixel(dev, kind, shape, builder="grid", how_a="dense", how_b="dense", grad=None, weight=1.0, out_scale=1.0,
              out_acc=0, npart=None):
    """grad: None (value only: grad and ws NULL), 0 (beta = 0) or 1 (beta = 1)"""
    a, b, value, bound, tol_v, g_ref, g_tol = pixel_ref(kind, builder, shape, weight)
    label = f"{kind} {shape} {builder} a={how_a} b={how_b} grad={grad} w={weight} s={out_scale} acc={out_acc}"
    gen = R.gen(9)
    A, Bt = place(a, how_a, dev), place(b, how_b, dev)
    d = desc4(KIND[kind], A.data_ptr(), Bt.data_ptr(), A.stride(), Bt.stride(), shape, weight=weight,
              out_scale=out_scale)
    out_prior = torch.randn(1, generator=gen) if out_acc else None
    grad_prior = torch.randn(shape, generator=gen) * float(g_ref.abs().max()) if grad == 1 else None
    out, got_g, n = launch(dev, d, out_prior=out_prior, grad_shape=shape if grad is not None else None,
                           grad_prior=grad_prior)
    assert npart is None or n == npart
    if kind == "ssim":  # the measured tolerance covers the value as stored; out_acc adds one rounding
        want = R.f32(out_scale) * value + (out_prior.double() if out_acc else 0)
        tol = abs(R.f32(out_scale)) * tol_v + (EPS * want.abs() if out_acc else 0)
    else:
        want, tol = R.stored(value, bound, out_scale, out_prior.double() if out_acc else None)
    close(f"{label} value", out, want, tol)
    if grad is not None:
        want_g, tol_g = R.accumulated(g_ref, g_tol, grad_prior)
        close(f"{label} grad", got_g, want_g, tol_g)


OPTIONS = {
    "value": dict(),
    "grad0": dict(grad=0),
    "grad1": dict(grad=1),
    "scaled": dict(grad=1, weight=0.37, out_scale=20.0, out_acc=1),
    "a_cl": dict(grad=0, how_a="cl"),
    "b_in": dict(grad=0, how_b="in"),
    "both": dict(grad=1, how_a="cl", how_b="in", weight=0.37),
    "swapped": dict(grad=0, how_a="in", how_b="cl"),
}


@pytest.mark.parametrize("opt", list(OPTIONS))
@pytest.mark.parametrize("kind", ["l1", "gdl", "ssim"])
def test_pixel_loss_options(dev, kind, opt):
    """(2, 3, 17, 23): one whole SSIM tile plus a 1-row / 7-column overhang; every option"""
    run_pixel(dev, kind, RAGGED, **OPTIONS[opt])


@pytest.mark.parametrize("builder", ["degenerate", "flat"])
@pytest.mark.parametrize("grad", [0, 1])
def test_ssim_special_inputs(dev, builder, grad):
    run_pixel(dev, "ssim", RAGGED, builder=builder, grad=grad)


@pytest.mark.parametrize("grad", [0, 1])
@pytest.mark.parametrize("shape,npart", [((1, 1, 5, 7), 1), ((1, 2, 16, 16), 2), ((1, 1, 33, 49), 12),
                                         ((4, 3, 65, 81), 360)])
def test_ssim_shapes(dev, shape, npart, grad):
    """image smaller than the window; exactly one tile; an overhang of 1 both ways after whole
    tiles; 360 partials for finalize_kernel's 256 threads"""
    run_pixel(dev, "ssim", shape, grad=grad, npart=npart)


@pytest.mark.parametrize("grad", [0, 1])
@pytest.mark.parametrize("kind,shape,npart", [("gdl", (1, 1, 2, 2), 1), ("l1", (1, 1, 2, 2), 1), ("l1", (1, 1, 1, 1), 1),
                                              ("l1", (1, 3, 1, 300), 1), ("l1", (2, 3, 300, 300), 264),
                                              ("gdl", (2, 3, 300, 300), 264)])
def test_l1_gdl_shapes(dev, kind, shape, npart, grad):
    run_pixel(dev, kind, shape, grad=grad, npart=npart)


def test_l1_past_the_grid_cap(dev):
    """4.32M elements want 2110 blocks of 2048 elements: the grid is capped at 2048 and strides"""
    run_pixel(dev, "l1", (1, 3, 1200, 1200), grad=0, npart=2048)


# ---------------- MSE ----------------
MSE_SHAPES = [((3, 3, 7, 9), 3), ((2, 3, 32, 64), 6), ((2, 1, 1, 2049), 4), ((2, 3, 419, 419), 512)]


@functools.lru_cache(maxsize=None)
def mse_ref(shape):
    a, b = R.mse_pair(shape, 40 + shape[-1])
    return a, b, R.mse(a, b)


@pytest.mark.parametrize("opt", ["dense", "acc_scaled", "a_cl", "b_in"])
@pytest.mark.parametrize("shape,npart", MSE_SHAPES)
def test_mse(dev, shape, npart, opt):
    """one short block per sample; 3 blocks per sample; a second block of one element; the
    256-blocks-per-sample cap.  out holds exactly B floats."""
    a, b, r = mse_ref(shape)
    A = place(a, "cl" if opt == "a_cl" else "dense", dev)
    Bt = place(b, "in" if opt == "b_in" else "dense", dev)
    scale = 3.0 if opt == "acc_scaled" else 1.0
    prior = torch.randn(shape[0], generator=R.gen(3)) if opt == "acc_scaled" else None
    d = desc4(L.LOSS_MSE, A.data_ptr(), Bt.data_ptr(), A.stride(), Bt.stride(), shape, out_scale=scale)
    out, _, n = launch(dev, d, nout=shape[0], out_prior=prior)
    assert n == npart
    want, tol = R.stored(r.value, r.bound, scale, prior.double() if prior is not None else None)
    close(f"mse {shape} {opt}", out, want, tol)


# ---------------- cross entropy ----------------
CE_OPTIONS = {
    "onehot": dict(grad=0),
    "value": dict(grad=None),
    "soft": dict(target="soft", grad=1, weight=0.37),
    "strided": dict(grad=0, how_a="cl", how_b="in", weight=0.37, out_scale=30.0, out_acc=1),
    "soft_strided": dict(target="soft", grad=0, how_a="in", how_b="cl"),
}


@functools.lru_cache(maxsize=None)
def ce_ref(shape, target, weight):
    logits = R.ce_logits(shape, 50 + shape[1])
    tgt = R.onehot_target(shape, 51) if target == "onehot" else R.soft_tied_target(shape, 51)
    return logits, tgt, R.ce(logits, tgt, weight)


@pytest.mark.parametrize("opt", list(CE_OPTIONS))
@pytest.mark.parametrize("shape", [(1, 2, 1, 1), (2, 20, 9, 13), (3, 5, 17, 31)])
def test_ce(dev, shape, opt):
    """logits of scale 30 (no max-subtraction overflows expf), one-hot and tied soft targets (the
    first maximum is the label), strided logits and targets, beta 0 / 1, weight and out_scale"""
    o = dict(target="onehot", how_a="dense", how_b="dense", weight=1.0, out_scale=1.0, out_acc=0)
    o.update(CE_OPTIONS[opt])
    logits, tgt, r = ce_ref(shape, o["target"], o["weight"])
    label = f"ce {shape} {opt}"
    gen = R.gen(5)
    A, Bt = place(logits, o["how_a"], dev), place(tgt, o["how_b"], dev)
    d = desc4(L.LOSS_CE, A.data_ptr(), Bt.data_ptr(), A.stride(), Bt.stride(), shape, weight=o["weight"],
              out_scale=o["out_scale"])
    out_prior = torch.randn(1, generator=gen) if o["out_acc"] else None
    grad_prior = torch.randn(shape, generator=gen) * float(r.grad.abs().max()) if o["grad"] == 1 else None
    out, got_g, _ = launch(dev, d, out_prior=out_prior, grad_shape=shape if o["grad"] is not None else None,
                           grad_prior=grad_prior)
    want, tol = R.stored(r.value, r.bound, o["out_scale"], out_prior.double() if o["out_acc"] else None)
    close(f"{label} value", out, want, tol)
    if o["grad"] is not None:
        want_g, tol_g = R.accumulated(r.grad, r.tol_grad, grad_prior)
        close(f"{label} grad", got_g, want_g, tol_g)
    if o["grad"] == 0:
        close(f"{label} grad rows sum to 0", got_g.double().sum(1), torch.zeros_like(r.tol_rowsum), r.tol_rowsum)


# ---------------- feature L1 over NHWC maps ----------------
# (element type, channels of the buffer, first channel, channels of the region)
L1NHWC_CASES = {
    "f32_dense": (torch.float32, 12, 0, 12),
    "f32_region": (torch.float32, 24, 4, 8),
    "bf16_dense": (torch.bfloat16, 16, 0, 16),       # the 16-byte kernel
    "bf16_stride20": (torch.bfloat16, 20, 0, 16),    # pixel stride not a multiple of 8
    "bf16_from_ch4": (torch.bfloat16, 24, 4, 16),    # region 8 bytes off a 16-byte boundary
    "bf16_ch12": (torch.bfloat16, 16, 0, 12),        # ch not a multiple of 8
}


@pytest.mark.parametrize("case", list(L1NHWC_CASES))
def test_l1nhwc(dev, case):
    """fp32 dense and as a channel region; bf16 dense (16-byte loads) and the three regions the
    dispatch has to send to the per-element kernel; then a second call with out_acc = 1, as the
    five VGG levels add into one scalar"""
    dt, C, c0, ch = L1NHWC_CASES[case]
    B, H, W = 2, 5, 7
    gen = R.gen(60 + C + ch)
    a = torch.randn((B, H, W, C), generator=gen).to(dt)
    b = torch.randn((B, H, W, C), generator=gen).to(dt)
    A, Bt = a.to(dev), b.to(dev)
    es = a.element_size()
    st = (H * W * C, 1, W * C, C)
    r = R.l1nhwc(a[..., c0:c0 + ch], b[..., c0:c0 + ch])
    d = desc4(L.LOSS_L1NHWC, A.data_ptr() + c0 * es, Bt.data_ptr() + c0 * es, st, st, (B, ch, H, W),
              dtype=L.F32 if dt == torch.float32 else L.BF16)
    out, _, _ = launch(dev, d)
    want, tol = R.stored(r.value, r.bound)
    close(f"l1nhwc {case}", out, want, tol)
    d.out_scale = 0.25
    out2, _, _ = launch(dev, d, out_prior=out)
    want2, tol2 = R.stored(r.value, r.bound, 0.25, out.double())
    close(f"l1nhwc {case} out_acc", out2, want2, tol2)


# ---------------- feature cosine ----------------
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("ch", [1, 3, 20, 64, 96, 512])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_cosnhwc(dev, dt, ch, layout):
    """1, 4, 32, 64, 64, 64 lanes per pixel; 70 pixels; NHWC strides as VGGCosineLoss passes them
    (sn, sc, sh, sw of the permuted view) and NCHW strides; weight 0.2"""
    B, H, W = 2, 5, 7
    gen = R.gen(70 + ch)
    a = torch.randn((B, ch, H, W), generator=gen).to(dt)
    b = (torch.randn((B, ch, H, W), generator=gen) + 0.5 * a.float()).to(dt)
    r = R.cosnhwc(a, b, 0.2)
    if layout == "nhwc":
        A, Bt = (t.permute(0, 2, 3, 1).contiguous().to(dev) for t in (a, b))
        st = (H * W * ch, 1, W * ch, ch)  # (sn, sc, sh, sw) of the (B, H, W, C) map
        if ch > 1:  # torch reports an arbitrary stride for a dimension of size 1
            sn, sh, sw, sc = A.stride()
            assert st == (sn, sc, sh, sw)
    else:
        A, Bt = a.to(dev), b.to(dev)
        st = A.stride()
    d = desc4(L.LOSS_COSNHWC, A.data_ptr(), Bt.data_ptr(), st, st, (B, ch, H, W),
              dtype=L.F32 if dt == torch.float32 else L.BF16, weight=0.2)
    out, _, _ = launch(dev, d)
    want, tol = R.stored(r.value, r.bound)
    close(f"cosnhwc {'f32' if dt == torch.float32 else 'bf16'} ch={ch} {layout}", out, want, tol)


def test_cosnhwc_zero_pixel_is_nan(dev):
    """one all-zero feature vector: 0 / 0, NaN in the reference and in the kernel (include/dvie.h)"""
    B, ch, H, W = 2, 20, 5, 7
    gen = R.gen(71)
    a, b = torch.randn((B, ch, H, W), generator=gen), torch.randn((B, ch, H, W), generator=gen)
    a[1, :, 2, 3] = 0
    assert torch.isnan(R.cosnhwc(a, b).value)
    A, Bt = a.to(dev), b.to(dev)
    d = desc4(L.LOSS_COSNHWC, A.data_ptr(), Bt.data_ptr(), A.stride(), Bt.stride(), (B, ch, H, W))
    lib = L.load()
    G = Guarded(dev)
    partial = nan_buf(G, (lib.dvie_loss_partial_count(ctypes.byref(d)),), torch.float64, "partial")
    out = G.put(torch.zeros(1), "out")
    d.partial, d.out = partial.data_ptr(), out.data_ptr()
    call(lib.dvie_loss, ctypes.byref(d), L.stream_ptr(dev))
    G.check()
    assert bool(torch.isnan(out).all())


# ---------------- IoU ----------------
def _iou_call(dev, kind, A, Bt, sa, sb, dims, ref, label):
    d = desc4(kind, A.data_ptr(), Bt.data_ptr(), sa, sb, dims)
    out, _, _ = launch(dev, d)
    close(label, out, ref.value, ref.tol)
    return float(out)


def test_iou_interior_slices(dev):
    """int64 label maps as interior slices of larger maps, a_sc = 0"""
    B, H, W = 2, 9, 13
    gen = R.gen(80)
    big_a = torch.randint(0, 20, (B, H + 4, W + 6), generator=gen)
    big_b = torch.where(torch.rand((B, H + 4, W + 6), generator=gen) < 0.7, big_a,
                        torch.randint(0, 20, (B, H + 4, W + 6), generator=gen))
    big_b[:, :2], big_b[:, :, :3] = -1, -1  # outside the slices nothing agrees
    big_b[:, 2 + H:], big_b[:, :, 3 + W:] = -1, -1
    a, b = big_a[:, 2:2 + H, 3:3 + W], big_b[:, 2:2 + H, 3:3 + W]
    A, Bt = big_a.to(dev)[:, 2:2 + H, 3:3 + W], big_b.to(dev)[:, 2:2 + H, 3:3 + W]
    sa = (A.stride(0), 0, A.stride(1), A.stride(2))
    ref = R.iou(a, b)
    assert 0.5 < float(ref.value) < 1
    _iou_call(dev, L.LOSS_IOU, A, Bt, sa, sa, (B, 1, H, W), ref, "iou interior slices")
    same = R.iou(a, a)
    assert _iou_call(dev, L.LOSS_IOU, A, A, sa, sa, (B, 1, H, W), same, "iou a == a") == 1.0


@pytest.mark.parametrize("case", ["ties", "nan_middle", "nan_first", "nan_both", "strided"])
def test_argmax_iou(dev, case):
    """the label is the first maximal channel, a NaN being the maximum (torch.argmax)"""
    shape = (2, 20, 9, 13)
    gen = R.gen(81)
    s = torch.randint(0, 3, shape, generator=gen).float()
    t = torch.where(torch.rand(shape, generator=gen) < 0.8, s, torch.randint(0, 3, shape, generator=gen).float())
    m = torch.rand((2, 9, 13), generator=gen) < 0.3
    m2 = torch.rand((2, 9, 13), generator=gen) < 0.3
    if case == "nan_middle":
        s[:, 7][m] = NAN
        s[:, 11][m2] = NAN  # a second NaN after the first does not take over
    elif case == "nan_first":
        s[:, 0][m] = NAN
        t[:, 0][m2] = NAN
    elif case == "nan_both":
        s[:, 7][m], t[:, 7][m] = NAN, NAN
        s[:, 3][m2], t[:, 12][m2] = NAN, NAN
    ref = R.argmax_iou(s, t)
    assert 0 < float(ref.value) < 1
    A, Bt = (place(s, "in", dev), place(t, "cl", dev)) if case == "strided" else (s.to(dev), t.to(dev))
    _iou_call(dev, L.LOSS_ARGMAX_IOU, A, Bt, A.stride(), Bt.stride(), shape, ref, f"argmax_iou {case}")


# ---------------- dvie_sum_f32 ----------------
@pytest.mark.parametrize("n", [1, 7, 64, 65])
def test_sum_f32(dev, n):
    """bit-equal to the float32 sum in index order; within (n - 1) EPS sum|x| of the fp64 sum"""
    x = R.mixed_magnitudes(n, 90 + n)
    seq, s64, tol = R.sum_f32(x)
    G = Guarded(dev)
    out = nan_buf(G, (1,), torch.float32, "out")
    X = x.to(dev)
    call(L.load().dvie_sum_f32, X.data_ptr(), n, out.data_ptr(), L.stream_ptr(dev))
    G.check()
    close(f"sum_f32 n={n} vs sequential fp32", out, torch.tensor([seq]), torch.zeros(1))
    close(f"sum_f32 n={n} vs fp64", out, torch.tensor([s64]), torch.tensor([tol]))


# ---------------- reparameterisation ----------------
@pytest.mark.parametrize("n", [1, 255, 257, 2048, 4096 * 256 + 3])
def test_reparam(dev, n):
    """one element, around one block, a whole number of blocks, past the 4096-block cap"""
    lib = L.load()
    st = L.stream_ptr(dev)
    D = R.reparam_inputs(n, n % 1000)
    r = R.reparam(D.mu, D.logvar, D.eps, D.gz)
    mu, lv, eps, gz = (t.to(dev) for t in (D.mu, D.logvar, D.eps, D.gz))
    G = Guarded(dev)
    z = nan_buf(G, (n,), torch.float32, "z")
    call(lib.dvie_reparam_fwd, mu.data_ptr(), lv.data_ptr(), eps.data_ptr(), z.data_ptr(), n, st)
    close(f"reparam n={n} z", z, r.z, r.bound_z)
    for beta in (0, 1):
        gmu = G.put(D.gmu0, f"gmu{beta}") if beta else nan_buf(G, (n,), torch.float32, "gmu0")
        glv = G.put(D.glv0, f"glv{beta}") if beta else nan_buf(G, (n,), torch.float32, "glv0")
        call(lib.dvie_reparam_bwd, lv.data_ptr(), eps.data_ptr(), gz.data_ptr(), gmu.data_ptr(), glv.data_ptr(), n, beta,
             st)
        want_mu, tol_mu = R.accumulated(r.gmu, torch.zeros_like(r.gmu), D.gmu0 if beta else None)
        want_lv, tol_lv = R.accumulated(r.glogvar, r.bound_glv, D.glv0 if beta else None)
        close(f"reparam n={n} gmu beta={beta}", gmu, want_mu, tol_mu)
        close(f"reparam n={n} glogvar beta={beta}", glv, want_lv, tol_lv)
    G.check()
    for t, src in ((mu, D.mu), (lv, D.logvar), (eps, D.eps), (gz, D.gz)):
        assert torch.equal(t.cpu(), src)


def test_reparam_empty(dev):
    """n = 0 returns OK and writes nothing"""
    lib = L.load()
    st = L.stream_ptr(dev)
    G = Guarded(dev)
    bufs = [nan_buf(G, (4,), torch.float32, name) for name in ("z", "gmu", "glogvar")]
    src = torch.ones(4, device=dev)
    call(lib.dvie_reparam_fwd, src.data_ptr(), src.data_ptr(), src.data_ptr(), bufs[0].data_ptr(), 0, st)
    call(lib.dvie_reparam_bwd, src.data_ptr(), src.data_ptr(), src.data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), 0,
         1, st)
    G.check()
    assert all(bool(torch.isnan(b).all()) for b in bufs)


# ---------------- rejected descriptors ----------------
REJECTED = {
    "gdl_h1": dict(kind=L.LOSS_GDL, dims=(2, 3, 1, 8)),
    "gdl_w1": dict(kind=L.LOSS_GDL, dims=(2, 3, 8, 1)),
    "cos_grad": dict(kind=L.LOSS_COSNHWC, grad=True),
    "iou_grad": dict(kind=L.LOSS_IOU, grad=True),
    "argmax_iou_grad": dict(kind=L.LOSS_ARGMAX_IOU, grad=True),
    "ssim_grad_no_ws": dict(kind=L.LOSS_SSIM, grad=True),
    "zero_w": dict(kind=L.LOSS_L1, dims=(2, 3, 8, 0)),
    "zero_batch": dict(kind=L.LOSS_SSIM, dims=(0, 3, 8, 8)),
    "unknown_kind": dict(kind=9),
    "negative_kind": dict(kind=-1),
}


@pytest.mark.parametrize("case", list(REJECTED))
def test_rejected_descriptors(dev, case):
    """host-side checks: a non-zero status, a message, nothing launched (every output buffer
    keeps its NaN fill and the guards their bytes)"""
    o = dict(dims=(2, 3, 8, 8), grad=False)
    o.update(REJECTED[case])
    lib = L.load()
    G = Guarded(dev)
    src = torch.zeros((2, 3, 8, 8), dtype=torch.float64, device=dev)  # large enough for any element type
    outs = [nan_buf(G, (2 * 3 * 8 * 8 * 3,), torch.float32, name) for name in ("out", "grad", "ws")]
    partial = nan_buf(G, (2048,), torch.float64, "partial")
    d = desc4(o["kind"], src.data_ptr(), src.data_ptr(), (192, 64, 8, 1), (192, 64, 8, 1), o["dims"])
    d.out, d.partial = outs[0].data_ptr(), partial.data_ptr()
    if o["grad"]:
        d.grad = outs[1].data_ptr()
    rc = lib.dvie_loss(ctypes.byref(d), L.stream_ptr(dev))
    assert rc != L.DVIE_OK
    assert len(lib.dvie_last_error()) > 0
    G.check()
    assert all(bool(torch.isnan(t).all()) for t in outs + [partial])
