"""Plain fp64 references of the loss and metric reductions (test infrastructure only): the nine
kinds of dvie_loss (L1, GDL, SSIM, MSE, CE, L1NHWC, COSNHWC, IOU, ARGMAX_IOU), dvie_sum_f32 and
the VAE reparameterisation of include/dvie.h, with the input builders and the error bounds the
op-level GPU tests (tests/test_gpu_loss_ops.py) compare under.  Nothing here touches libdvie.

References.  oracle/losses.py is dtype-agnostic: l1_loss, gdl_loss, ssim_loss, seg_ce and the
per-sample MSE inside psnr run on `.double()` inputs, torch autograd gives d loss / d a.  The
metrics and the reparameterisation are a few lines of fp64 torch here.  Every function takes the
exact values the kernel sees (a bf16 tensor as its values upcast, a `float` field of the
descriptor as that float, `f32`).

Bounds.  EPS = 2^-24 is the fp32 unit roundoff.  The kernels evaluate each term in fp32, add the
terms in double (per thread, per block, over the partials: at most a few dozen additions on any
path, allowed for by DACC = 2^-40 relative to the sum of the term magnitudes) and round the
result to fp32 once.  A bound follows those roundings and is built from reference quantities
only, never from a kernel's output; the derivations are in the docstrings.  `stored()` adds what
happens to the value afterwards (the fp32 rounding, the product with out_scale, the addition to
*out under out_acc), `accumulated()` the fp32 addition of a gradient to what the buffer held.

SSIM is the exception (`ssim_tolerance`): the kernel's separable 11 + 11 tap sums are ordered
differently from conv2d's 121 taps and E[x^2] - mu^2 cancels, so the tolerance is measured on the
reference's own arithmetic: 8 * max|fp32 CPU oracle - fp64 oracle| on the same input, plus
4 EPS max|ref|.  The fp32 oracle is the reference project's formula, not the code under test.
"""
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import losses as OL

ACC = torch.float64
EPS = 2.0 ** -24
DACC = 2.0 ** -40
F32_TINY = 2.0 ** -126  # smallest normal fp32: a flushed subnormal is off by less than this
SSIM_FACTOR = 8.0
TILE = 16  # the SSIM kernel's output tile edge


def f32(v):
    """the value a C `float` holds for the Python number v, as a Python float"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def ulp32(v):
    """the spacing of fp32 numbers at |v| (0 for v == 0)"""
    v = abs(float(v))
    return 0.0 if v == 0.0 else 2.0 ** (max(math.floor(math.log2(v)), -126) - 23)


def _ns(**kw):
    return types.SimpleNamespace(**kw)


# ---------------- input builders ----------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def grid_image(shape, g):
    """fp32 values k / 64, k in [-64, 64]: every a - b and every difference of differences is an
    exact multiple of 1/64 below 2^3, so exact in fp32, and either 0 or at least 1/64"""
    return torch.randint(-64, 65, shape, generator=g).float() / 64


def grid_pair(shape, seed):
    g = gen(seed)
    return grid_image(shape, g), grid_image(shape, g)


def ssim_near_degenerate(shape, seed=7):
    """prediction a small negative constant plus noise, target positive: 2 mu1 mu2 + C1 and
    2 sigma12 + C2 cross zero at some pixels"""
    g = gen(seed)
    gt = torch.rand(shape, generator=g)
    pred = -0.02 + 0.003 * torch.randn(shape, generator=g)
    return pred, gt


def ssim_flat(shape):
    """constant 0.7, one pixel of the prediction raised by 1/64: E[x^2] - mu^2 cancels in fp32"""
    b = torch.full(shape, 0.7)
    a = b.clone()
    a[..., shape[-2] // 2, shape[-1] // 2] += 1.0 / 64
    return a, b


def mse_pair(shape, seed):
    """sample i's error is (i + 1) times a grid image, so no two samples share an MSE"""
    a, e = grid_pair(shape, seed)
    scale = torch.arange(1, shape[0] + 1, dtype=torch.float32).view(-1, 1, 1, 1)
    return a, a - scale * e / 8


def ce_logits(shape, seed, scale=30.0):
    return torch.randn(shape, generator=gen(seed)) * scale


def onehot_target(shape, seed):
    b, c, h, w = shape
    lab = torch.randint(0, c, (b, h, w), generator=gen(seed))
    return F.one_hot(lab, c).permute(0, 3, 1, 2).float().contiguous()


def soft_tied_target(shape, seed):
    """values k / 4, k in [0, 3]: with more than a few channels nearly every pixel's maximum is
    attained more than once; the label is the first (torch.argmax)"""
    return torch.randint(0, 4, shape, generator=gen(seed)).float() / 4


def channels_last(t):
    """the same NCHW values over NHWC memory"""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


PAD_VALUE = 1000.0


def interior(t):
    """t as the slice big[:, 1:1+C, 2:2+H, 3:3+W] of a larger tensor whose other elements hold
    PAD_VALUE; returns (view, big)"""
    b, c, h, w = t.shape
    big = torch.full((b, c + 2, h + 4, w + 6), PAD_VALUE, dtype=t.dtype)
    view = big[:, 1:1 + c, 2:2 + h, 3:3 + w]
    view.copy_(t)
    return view, big


def strided(t, how):
    """how: 'dense', 'cl' (channels-last view) or 'in' (interior slice)"""
    if how == "cl":
        return channels_last(t)
    if how == "in":
        return interior(t)[0]
    return t.contiguous()


# ---------------- what happens to a value or gradient after the reduction ----------------
def stored(value, bound, out_scale=1.0, prior=None):
    """value: the fp64 reference of the reduction; bound: the error of the double the kernel
    holds before the store.  finalize_kernel: v = (float) value (EPS |value|);
    vscale * v (EPS |product|); with out_acc the fp32 sum with the prior (EPS |total|).
    -> (expected out, tolerance)"""
    value = torch.as_tensor(value, dtype=ACC)
    s = f32(out_scale)
    scaled = s * value
    tol = abs(s) * (torch.as_tensor(bound, dtype=ACC) + EPS * value.abs()) + EPS * scaled.abs()
    if prior is None:
        return scaled, tol
    total = scaled + torch.as_tensor(prior, dtype=ACC)
    return total, tol + EPS * total.abs()


def accumulated(grad, tol, prior=None):
    """beta = 1: grad[e] = grad[e] + v in fp32 -> (expected, tolerance)"""
    if prior is None:
        return grad, tol
    total = grad + prior.to(ACC)
    return total, tol + EPS * total.abs()


# ---------------- L1, GDL, MSE ----------------
def _autograd(fn, a, b, dtype=ACC):
    a = a.to(dtype).clone().requires_grad_(True)
    v = fn(a, b.to(dtype))
    v.backward()
    return v.detach(), a.grad


def l1(a, b, weight=1.0):
    """value: fabsf(a - b) per element, one rounding: EPS mean|d| (0 on grid inputs, kept general).
    grad = weight * (sgn(d) / (float) N): the fp32 quotient and the fp32 product, half an ulp
    each: (2 EPS + EPS^2) |ref|, one ulp of weight / N."""
    value, grad = _autograd(OL.l1_loss, a, b)
    w = f32(weight)
    d = (a.to(ACC) - b.to(ACC)).abs()
    return _ns(value=value, bound=EPS * d.mean() + DACC * value.abs(), grad=w * grad,
               tol_grad=2 * EPS * (1 + EPS) * (w * grad).abs())


def gdl(a, b, weight=1.0):
    """value: dx = (a[x+1] - a[x]) - (b[x+1] - b[x]) in fp32, three roundings (none on grid
    inputs): EPS (|da| + |db| + |dx|) per term, the terms |dx| / (2 nx) formed and added in double.
    grad = weight * (float)(gx / (2 nx) + gy / (2 ny)) with gx, gy sums of up to two signs each,
    the sum in double: one rounding and the product, (2 EPS + EPS^2) of the magnitude of the
    terms, weight * (cx / (2 nx) + cy / (2 ny)), cx / cy the number of non-zero signs meeting at
    the element (the magnitude, not |ref|: the double sum is rounded once, but a reference formed
    in fp32 rounds every term)."""
    value, grad = _autograd(OL.gdl_loss, a, b)
    w = f32(weight)
    a, b = a.to(ACC), b.to(ACC)
    B, C, H, W = a.shape
    nx, ny = B * C * H * (W - 1), B * C * (H - 1) * W
    dax, dbx = a[..., 1:] - a[..., :-1], b[..., 1:] - b[..., :-1]
    day, dby = a[..., 1:, :] - a[..., :-1, :], b[..., 1:, :] - b[..., :-1, :]
    bound = EPS * ((dax.abs() + dbx.abs() + (dax - dbx).abs()).sum() / (2 * nx)
                   + (day.abs() + dby.abs() + (day - dby).abs()).sum() / (2 * ny)) + DACC * value.abs()
    mag = torch.zeros_like(a)
    sx, sy = torch.sign(dax - dbx).abs() / (2 * nx), torch.sign(day - dby).abs() / (2 * ny)
    mag[..., :-1] += sx
    mag[..., 1:] += sx
    mag[..., :-1, :] += sy
    mag[..., 1:, :] += sy
    return _ns(value=value, bound=bound, grad=w * grad, tol_grad=(2 * EPS * (1 + EPS) + DACC) * abs(w) * mag)


def mse(a, b):
    """per sample mean((a - b)^2): d rounded (2 EPS d^2), the square rounded (EPS d^2), added in
    double: 3 EPS mean(d^2) per sample"""
    d2 = (a.to(ACC) - b.to(ACC)) ** 2
    value = d2.reshape(a.shape[0], -1).mean(1)
    return _ns(value=value, bound=(3 * EPS + DACC) * value)


# ---------------- SSIM ----------------
def ssim_parts(a, b, pad_mode="zero"):
    """the reference formula (oracle.losses.ssim_value) with E[a^2]'s input as a leaf of its own:
    after backward `sq.grad` is G * (dL / dE11), the factor of 2 a in the gradient.
    pad_mode 'replicate' is the edge-replicating mutant."""
    c = a.shape[1]
    w = OL.gaussian_window(11, dtype=a.dtype).to(a.dtype).expand(c, 1, 11, 11).contiguous()

    def conv(x):
        if pad_mode == "zero":
            return F.conv2d(x, w, padding=5, groups=c)
        return F.conv2d(F.pad(x, (5, 5, 5, 5), mode="replicate"), w, groups=c)

    sq = (a * a).detach().requires_grad_(True)
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(sq) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return 1 - m.mean(), sq


def ssim(a, b, dtype=ACC):
    """(1 - mean ssim, d / d a) of the oracle in `dtype`"""
    return _autograd(OL.ssim_loss, a, b, dtype)


def ssim_mutant(a, b, which):
    """deliberately wrong fp64 SSIM references -> (value, grad).
    'replicate': edge-replicate instead of zero padding;
    'drop_beta_last_row': the gradient without its 2 a (G * beta) term on the rows of the last,
    partial tile row (H not a multiple of 16)"""
    x = a.to(ACC).clone().requires_grad_(True)
    if which == "replicate":
        v, sq = ssim_parts(x, b.to(ACC), "replicate")
        v.backward()
        return v.detach(), x.grad + 2 * x.detach() * sq.grad
    assert which == "drop_beta_last_row" and a.shape[-2] % TILE
    v, sq = ssim_parts(x, b.to(ACC))
    v.backward()
    full = x.grad + 2 * x.detach() * sq.grad
    y0 = a.shape[-2] // TILE * TILE
    full[..., y0:, :] -= (2 * x.detach() * sq.grad)[..., y0:, :]
    return v.detach(), full


def ssim_tolerance(a, b, weight=1.0):
    """-> namespace(value, grad (times weight), tol_value, tol_grad, dist_value, dist_grad):
    tol = SSIM_FACTOR * max|fp32 oracle - fp64 oracle| + 4 EPS max|ref| (module docstring), one
    number for the value and one for every element of the gradient; the weight multiplies the
    gradient and its tolerance (one more fp32 product, inside the 4 EPS)"""
    v64, g64 = ssim(a, b, ACC)
    v32, g32 = ssim(a, b, torch.float32)
    w = f32(weight)
    dv = float((v32.double() - v64).abs())
    dg = float((g32.double() - g64).abs().max())
    tol_v = SSIM_FACTOR * dv + 4 * EPS * float(v64.abs())
    tol_g = abs(w) * (SSIM_FACTOR * dg + 4 * EPS * float(g64.abs().max()))
    return _ns(value=v64, grad=w * g64, tol_value=torch.tensor(tol_v, dtype=ACC),
               tol_grad=torch.full_like(g64, tol_g), dist_value=dv, dist_grad=dg, v32=v32, g32=g32,
               gmax=float(g64.abs().max()))


# ---------------- cross entropy ----------------
def ce(logits, target, weight=1.0, last_max=False):
    """mean_pix(logsumexp(a) - a[label]), label = the first maximum of the target
    (last_max = True: the mutant that takes the last one).

    factor = (c + 8 + max|a - m|) EPS is the relative error of s = sum expf(a - m) in fp32
    (gan_ref.softmax_fwd: the subtraction's rounding is relative in exp, expf, c sequential
    additions), hence the absolute error of logf(s); logf itself and the sums m + log s and
    lse - a[label] round once each: bound_px = factor + EPS (2 |log s| + |lse| + |value_px|).
    grad = (p - onehot) * inv, inv = weight / (float) npx: p = expf(a - m) / s carries
    factor + 2 EPS relative, the subtraction, inv and the product one rounding each:
    inv (factor + 2 EPS) p + 3 EPS |ref|, plus inv * 2^-126 where expf flushes a subnormal."""
    value, grad = _autograd(OL.seg_ce, logits, target)
    a, t = logits.to(ACC), target.to(ACC)
    B, C, H, W = a.shape
    npx = B * H * W
    w = f32(weight)
    label = t.argmax(1)
    if last_max:
        label = C - 1 - t.flip(1).argmax(1)
        x = a.clone().requires_grad_(True)
        value = F.cross_entropy(x, label)
        value.backward()
        value, grad = value.detach(), x.grad
    m = a.max(1, keepdim=True).values
    e = torch.exp(a - m)
    s = e.sum(1, keepdim=True)
    p = e / s
    lse = m + s.log()
    px = (lse - a.gather(1, label.unsqueeze(1))).abs()
    factor = (C + 8 + (a - m).abs().max(1, keepdim=True).values) * EPS
    bound_px = factor + EPS * (2 * s.log().abs() + lse.abs() + px)
    inv = abs(w) / npx
    tol_grad = inv * (factor + 2 * EPS) * p + 3 * EPS * (w * grad).abs() + inv * F32_TINY
    return _ns(value=value, bound=bound_px.mean() + DACC * px.mean(), grad=w * grad, tol_grad=tol_grad,
               tol_rowsum=tol_grad.sum(1))


# ---------------- feature L1 and cosine over NHWC maps ----------------
def l1nhwc(a, b):
    """a, b: the stored values, any layout.  fp32 kernel: fabsf(a - b), one rounding; bf16
    kernels: the difference of two bf16 values is exact in fp32 unless their exponents are more
    than 16 apart (then one rounding), and the 16-byte kernel adds 8 of them in fp32 before the
    double (7 roundings of a partial sum): 9 EPS mean|d| covers the three kernels."""
    d = (a.to(ACC) - b.to(ACC)).abs()
    value = d.mean()
    return _ns(value=value, bound=(9 * EPS + DACC) * value)


def cos_lanes(ch):
    """lanes per pixel of cosnhwc_kernel: ch rounded up to a power of two, at most 64"""
    L = 1
    while L < ch and L < 64:
        L <<= 1
    return L


def cosnhwc(a, b, weight=1.0, ch_limit=None):
    """a, b: (B, C, H, W) stored values.  weight * mean_pix(a.b / (|a| |b|)); NaN where a pixel's
    feature vector is all zero, as the reference's 0 / 0.  ch_limit: the mutant that leaves out
    the channels from ch_limit on.

    Each of L lanes adds T = ceil(ch / L) products sequentially in fp32 and log2 L shuffle steps
    join them: gamma = (T + log2 L + 1) EPS relative to sum|a_c b_c| for the dot product and to
    the sums of squares themselves.  sqrt halves gamma and rounds (twice), the product and the
    quotient round: bound_px = gamma sum|a_c b_c| / (|a| |b|) + (gamma + 4 EPS) |cos|."""
    a, b = a.to(ACC), b.to(ACC)
    ch = a.shape[1]
    w = f32(weight)
    if ch_limit is not None:
        a, b = a[:, :ch_limit], b[:, :ch_limit]
    na, nb = (a * a).sum(1).sqrt(), (b * b).sum(1).sqrt()
    cos = (a * b).sum(1) / (na * nb)
    L = cos_lanes(ch)
    gamma = (math.ceil(ch / L) + math.log2(L) + 1) * EPS
    bound_px = gamma * (a * b).abs().sum(1) / (na * nb) + (gamma + 4 * EPS) * cos.abs()
    value = w * cos.mean()
    return _ns(value=value, bound=abs(w) * bound_px.mean() + DACC * abs(w) * cos.abs().mean())


# ---------------- IoU ----------------
def iou(la, lb):
    """fraction of agreeing labels: an integer count over the pixel count, rounded to fp32 once"""
    value = (la == lb).to(ACC).mean()
    return _ns(value=value, tol=torch.tensor(ulp32(value), dtype=ACC))


def argmax_iou(sa, sb):
    """torch.argmax on the fp32 scores: the first maximum, NaN being the maximum"""
    return iou(torch.argmax(sa, 1), torch.argmax(sb, 1))


# ---------------- dvie_sum_f32 ----------------
def sum_f32(x):
    """-> (the float32 sum in index order, the fp64 sum, (n - 1) EPS sum|x|)"""
    v = x.numpy().astype(np.float32)
    s = np.float32(0)
    for t in v:
        s = np.float32(s + t)
    return float(s), float(x.double().sum()), (len(v) - 1) * EPS * float(x.double().abs().sum()) + EPS * abs(float(s))


def mixed_magnitudes(n, seed):
    """values whose exponents spread over 2^-12 .. 2^12, both signs: the float32 sum depends on
    the order of the additions"""
    g = gen(seed)
    return torch.randn(n, generator=g) * 2.0 ** torch.randint(-12, 13, (n,), generator=g).float()


# ---------------- reparameterisation ----------------
def reparam_inputs(n, seed):
    g = gen(seed)
    return _ns(mu=torch.randn(n, generator=g), logvar=torch.rand(n, generator=g) * 10 - 6,
               eps=torch.randn(n, generator=g), gz=torch.randn(n, generator=g),
               gmu0=torch.randn(n, generator=g), glv0=torch.randn(n, generator=g))


def reparam(mu, logvar, eps, gz, half=0.5):
    """z = eps * exp(0.5 logvar) + mu; gmu = gz; glogvar = gz * eps * 0.5 * exp(0.5 logvar)
    (half = 1: the mutant without the factor).

    0.5 * logvar is exact.  expf is within 2 ulp (4 EPS relative); the product and the sum round
    once each (fused or not): bound_z = 6 EPS |eps std| + EPS |z|.  glogvar: three more products
    (the one with 0.5 is exact): bound_glv = 8 EPS |ref|.  gmu is a copy."""
    mu, logvar, eps, gz = mu.to(ACC), logvar.to(ACC), eps.to(ACC), gz.to(ACC)
    std = torch.exp(0.5 * logvar)
    z = eps * std + mu
    glv = gz * eps * half * std
    return _ns(z=z, gmu=gz, glogvar=glv, bound_z=6 * EPS * (eps * std).abs() + EPS * z.abs(),
               bound_glv=8 * EPS * glv.abs())
