"""Plain fp64 references of the GAN-side ops (test infrastructure only): BatchNorm, the
discriminator head, the channel softmax, SpectralNorm and the fused Adam / Adamax steps of
include/dvie.h, in torch float64 on the CPU, each with the elementwise error bound the op-level
GPU tests (tests/test_gpu_gan_ops.py) compare under.  Nothing here touches libdvie.

Every function takes the exact values the kernel sees: a bf16 tensor is passed as its bf16
values upcast, a `float` field of a descriptor (eps, momentum, alpha) or a constant the launcher
casts to float (Adam's b1, b2, eps, wd) as that float (`f32`).

Error bounds.  EPS = 2^-24 is the fp32 unit roundoff.  BF16_EPS = 2^-8 is the bf16 one: bf16
keeps 8 significant bits, its values in [1, 2) are 2^-7 apart, and round-to-nearest is off by
up to half of that, 2^-8 relative just above a power of two (2^-9 is reached only in the upper
half of a binade; a correctly rounding store was measured at 1.97 * 2^-9).  A
bound follows the roundings the kernel's arithmetic performs (the kernel sources say which
quantities are fp32 and which fp64) and is built from reference quantities only, never from a
kernel's output.  A comparison is |got - ref| <= K * bound + (the rounding of the stored
output), K being the constant next to each function; the derivations are in the docstrings.
"""
import math
import types

import torch
import torch.nn.functional as F

ACC = torch.float64
EPS = 2.0 ** -24
BF16_EPS = 2.0 ** -8

K_BN_FWD = 8.0
K_BN_DX = 8.0
K_BN_DGAMMA = 4.0
K_HEAD = 1.0
K_SOFTMAX = 1.0
K_SN = 1.0
K_OPT = 1.0


def f32(v):
    """the value a C `float` holds for the Python number v, as a Python float"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def store_eps(dtype):
    """unit roundoff of a stored output of that element type"""
    return BF16_EPS if dtype == torch.bfloat16 else EPS


def _ns(**kw):
    return types.SimpleNamespace(**kw)


# ---------------- BatchNorm ----------------
def bn_fwd(x, gamma=None, beta=None, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-5,
           lrelu=False, alpha=0.2):
    """x: (rows, c).  Training: batch mean, biased variance for the normalisation, running
    statistics (if given) updated with `momentum` and the unbiased variance (rows == 1: the
    biased one, 0 -- the kernel's defined value where nn.BatchNorm2d refuses the input);
    eval: the running statistics.  y = act(gamma * (x - mean) * invstd + beta).

    bound_y (K_BN_FWD = 8): the kernel rounds mean, invstd, scale = gamma * invstd and
    shift = beta - mean * scale to fp32 and evaluates x * scale + shift in fp32: relative 2 EPS on
    scale (3 with the product's own rounding), 4 EPS on mean * scale, one each on shift and on
    the sum, one more for the LeakyReLU product: at most 5..6 EPS times
    |x scale| + |mean scale| + |beta| + |y|.  A LeakyReLU branch flip moves y by at most
    (1 - alpha) |pre| with |pre| below its own error, so it is inside the bound.
    mean / invstd / running statistics: fp64 arithmetic, one rounding (2 EPS |ref| allowed)."""
    x = x.to(ACC)
    rows, c = x.shape
    eps, momentum, alpha = f32(eps), f32(momentum), f32(alpha)
    new_rm = new_rv = None
    if training:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        if running_mean is not None:
            unb = var * rows / (rows - 1) if rows > 1 else var
            new_rm = (1.0 - momentum) * running_mean.to(ACC) + momentum * mean
            new_rv = (1.0 - momentum) * running_var.to(ACC) + momentum * unb
    else:
        mean, var = running_mean.to(ACC), running_var.to(ACC)
    invstd = 1.0 / torch.sqrt(var + eps)
    gam = gamma.to(ACC) if gamma is not None else torch.ones(c, dtype=ACC)
    bet = beta.to(ACC) if beta is not None else torch.zeros(c, dtype=ACC)
    scale = gam * invstd
    pre = (x - mean) * scale + bet
    y = torch.where(pre > 0, pre, pre * alpha) if lrelu else pre
    bound_y = EPS * ((x * scale).abs() + (mean * scale).abs() + bet.abs() + y.abs())
    return _ns(y=y, mean=mean, var=var, invstd=invstd, running_mean=new_rm, running_var=new_rv, bound_y=bound_y)


def bn_bwd(x, g, gamma, mean, invstd):
    """Training-mode BatchNorm backward from the exact fp64 mean and invstd of bn_fwd; g is the
    gradient of the pre-activation output.  dx = A (g - mg) + B (x - mean) with A = gamma invstd,
    B = -A invstd^2 sum(g (x - mean)) / rows, mg = mean(g); dgamma = invstd sum(g (x - mean));
    dbeta = sum(g).

    bound_dx (K_BN_DX = 8): the kernel evaluates the same expression in fp64 from the fp32
    mean32 = mean (1 + d1) and invstd32 = invstd (1 + d2), |d| <= EPS.  d2 gives
    EPS |A| (|g| + |mg|) + 3 EPS |B| |x - mean|; d1 moves x - mean32 by EPS |mean| (the term
    EPS |B| |mean|) and moves the fp64 sum of g (x - mean32) by EPS |mean| |sum g|, hence B by
    EPS |A| invstd^2 |mean| |mg|, which multiplies |x - mean|.  That last term is what a bound of
    only EPS (|A| (|g| + |mg|) + |B| (|x - mean| + |mean|)) leaves out; it is the largest one in
    a channel whose |mean| is many standard deviations.
    bound_dgamma (K_BN_DGAMMA = 4), to which the caller adds EPS |stored dgamma|: d2 on invstd
    and d1 through the sum as above.  dbeta is an fp64 sum rounded once."""
    x, g = x.to(ACC), g.to(ACC)
    rows, c = x.shape
    gam = gamma.to(ACC) if gamma is not None else torch.ones(c, dtype=ACC)
    xc = x - mean
    sg, sgc = g.sum(0), (g * xc).sum(0)
    mg = sg / rows
    A = gam * invstd
    B = -A * invstd ** 2 * sgc / rows
    dx = A * (g - mg) + B * xc
    bound_dx = EPS * (A.abs() * (g.abs() + mg.abs()) + B.abs() * (xc.abs() + mean.abs())
                      + A.abs() * invstd ** 2 * mean.abs() * mg.abs() * xc.abs())
    dgamma = sgc * invstd
    bound_dgamma = EPS * (invstd * (g.abs() * xc.abs()).sum(0) + invstd * mean.abs() * sg.abs())
    return _ns(dx=dx, dgamma=dgamma, dbeta=sg, bound_dx=bound_dx, bound_dgamma=bound_dgamma)


# ---------------- discriminator head ----------------
def head_fwd(x, pool):
    """x: NHWC (n, h, w, c).  AvgPool2d(pool) of the NCHW tensor, then view(-1, c).mean(1) over
    its NCHW-flat order: unless the pooled map is 1x1, a group of c consecutive pooled values
    mixes pixels of several channels, not the channels of one pixel.

    bound (K_HEAD = 1): a sequential fp32 sum of pool^2 terms ((pool^2 - 1) EPS sum|x|), the
    fp32 division, and the fp64 group mean rounded once: (pool^2 + 2) EPS times the group mean
    of avgpool(|x|)."""
    x = x.to(ACC)
    c = x.shape[3]
    xn = x.permute(0, 3, 1, 2)
    out = F.avg_pool2d(xn, pool).reshape(-1, c).mean(1)
    bound = (pool * pool + 2) * EPS * F.avg_pool2d(xn.abs(), pool).reshape(-1, c).mean(1)
    return _ns(out=out, bound=bound)


def head_bwd(gout, n, h, w, c, pool):
    """The adjoint of head_fwd applied to gout (n * hp * wp values), written out: NHWC
    (n, h, w, c), zero past the floor(h / pool) * pool crop.

    bound (K_HEAD = 1): gout times the fp32 constant 1 / (c pool^2) (one rounding) in one fp32
    product: 3 EPS |ref| allowed; the caller adds the store / accumulate roundings."""
    hp, wp = h // pool, w // pool
    gp = (gout.to(ACC).reshape(-1).repeat_interleave(c) / c).reshape(n, c, hp, wp)
    full = torch.zeros((n, c, h, w), dtype=ACC)
    full[:, :, :hp * pool, :wp * pool] = gp.repeat_interleave(pool, 2).repeat_interleave(pool, 3) / (pool * pool)
    gx = full.permute(0, 2, 3, 1).contiguous()
    return _ns(gx=gx, bound=3 * EPS * gx.abs())


# ---------------- channel softmax ----------------
def softmax_fwd(x):
    """x: NCHW.  factor (n, 1, h, w) = (c + 8 + max|x - m|) EPS is the relative bound of the
    fp32 evaluation: x - m rounded (EPS |x - m| absolute in the exponent = relative in exp), expf,
    a sequential sum of c terms, the reciprocal and the product.  bound = factor * y
    (K_SOFTMAX = 1)."""
    x = x.to(ACC)
    c = x.shape[1]
    m = x.max(1, keepdim=True).values
    e = torch.exp(x - m)
    y = e / e.sum(1, keepdim=True)
    factor = (c + 8 + (x - m).abs().max(1, keepdim=True).values) * EPS
    return _ns(y=y, factor=factor, bound=factor * y)


def softmax_bwd(y, gy, factor):
    """gx = y (gy - sum_c gy y) from the y the kernel is given.  bound = factor * y * (|gy| +
    sum|gy y|) with the forward's factor (the dot product is a sequential fp32 sum of c
    products; then one subtraction and one product)."""
    y, gy = y.to(ACC), gy.to(ACC)
    dot = (gy * y).sum(1, keepdim=True)
    gx = y * (gy - dot)
    bound = factor * y * (gy.abs() + (gy * y).abs().sum(1, keepdim=True))
    return _ns(gx=gx, bound=bound)


# ---------------- SpectralNorm ----------------
def _l2normalize(x):
    return x / (x.norm() + 1e-12)


def sn_fwd(w, u, v, power_iterations):
    """w: (h, width); u (h), v (width) the given fp32 vectors.  `power_iterations` times
    v = l2normalize(W^T u); u = l2normalize(W v); then sigma = u . (W v), w_eff = W / sigma."""
    w, u, v = w.to(ACC), u.to(ACC), v.to(ACC)
    for _ in range(power_iterations):
        v = _l2normalize(w.t() @ u)
        u = _l2normalize(w @ v)
    sigma = u.dot(w @ v)
    return _ns(sigma=sigma, u=u, v=v, w_eff=w / sigma)


def sn_weff(w, sigma):
    """w_eff from the sigma the kernel saved: one fp32 division (2 EPS |ref| allowed)"""
    ref = w.to(ACC) / float(sigma)
    return _ns(w_eff=ref, bound=2 * EPS * ref.abs())


def sn_bwd(w, g_eff, sigma, u, v):
    """Backward of w / sigma, sigma = u . (W v), from the kernel's saved state (sigma, u, v), so a
    pure function of its inputs: gs = -sum(g_eff W) / sigma^2; g_bar = g_eff / sigma + gs u v^T;
    g_u = gs W v; g_v = gs W^T u.

    Bounds (K_SN = 1): gs is an fp64 sum rounded to fp32, W v and W^T u likewise; then fp32:
    one division, two products and a sum for g_bar (4 EPS (|g_eff / sigma| + |gs u_i v_j|)), one
    product for g_u / g_v (4 EPS |ref| allowed).  The caller adds the accumulate rounding."""
    w, g_eff, u, v = w.to(ACC), g_eff.to(ACC), u.to(ACC), v.to(ACC)
    sigma = float(sigma)
    gs = -(g_eff * w).sum() / (sigma * sigma)
    rank1 = gs * torch.outer(u, v)
    g_bar = g_eff / sigma + rank1
    g_u, g_v = gs * (w @ v), gs * (w.t() @ u)
    return _ns(g_bar=g_bar, g_u=g_u, g_v=g_v, bound_bar=4 * EPS * ((g_eff / sigma).abs() + rank1.abs()),
               bound_u=4 * EPS * g_u.abs(), bound_v=4 * EPS * g_v.abs())


# ---------------- optimizers ----------------
def adam(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
    """torch 1.0.1 Adam at integer step `step`: g += wd p; m = b1 m + (1 - b1) g;
    v = b2 v + (1 - b2) g^2; p -= step_size m / (sqrt(v) + eps),
    step_size = lr sqrt(1 - b2^step) / (1 - b1^step).  b1, b2, eps, wd act elementwise as
    floats (f32); step_size comes from the doubles, as in the kernel.

    Bounds (K_OPT = 1), w = 1 - b1 (exact in fp32), dg = EPS (|g| + |wd p|) the error of the
    decayed gradient (its product and sum, fused or not; 0 without weight decay):
      m: the products b1 m and w g and their sum, one rounding each:
         EPS (|b1 m| + |w g| + |m_new|) + w dg.  (2 EPS |m_new| alone misses the two product
         roundings, which are all that is left when b1 m and w g cancel: that bound is exceeded
         by four orders of magnitude among 4M random elements.)
      v: EPS (|b2 v| + 2 (1 - b2) g^2 + |v_new|) + 2 (1 - b2) |g| dg.
      p: 4 EPS (|p| + |update|) for the fp32 step_size, sqrt, sum, division, product and the
         final subtraction, plus the bounds of m and v carried through:
         step_size bound_m / (sqrt(v) + eps) + |update| bound_v / (2 sqrt(v) (sqrt(v) + eps))."""
    p, g, m, v = p.to(ACC), g.to(ACC), m.to(ACC), v.to(ACC)
    fb1, fb2, feps, fwd = f32(b1), f32(b2), f32(eps), f32(wd)
    gr = g + fwd * p
    w1, w2 = 1.0 - fb1, 1.0 - fb2
    mn = fb1 * m + w1 * gr
    vn = fb2 * v + w2 * gr * gr
    step_size = lr * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)
    den = vn.sqrt() + feps
    upd = step_size * mn / den
    dg = EPS * (gr.abs() + (fwd * p).abs()) if fwd != 0.0 else torch.zeros_like(gr)
    bound_m = EPS * ((fb1 * m).abs() + (w1 * gr).abs() + mn.abs()) + w1 * dg
    bound_v = EPS * ((fb2 * v).abs() + 2 * w2 * gr * gr + vn.abs()) + 2 * w2 * gr.abs() * dg
    bound_p = (4 * EPS * (p.abs() + upd.abs()) + step_size * bound_m / den
               + upd.abs() * bound_v / (2 * vn.sqrt().clamp_min(1e-300) * den))
    return _ns(p=p - upd, m=mn, v=vn, bound_p=bound_p, bound_m=bound_m, bound_v=bound_v)


def adamax(p, g, m, u, step, lr, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
    """torch.optim.Adamax at integer step `step`: g += wd p; m = m + (1 - b1) (g - m);
    u = max(b2 u, |g| + eps); p -= clr m / u, clr = lr / (1 - b1^step).

    Bounds (K_OPT = 1), w = 1 - b1, dg as in adam: m: g - m, its product with w and the sum, one
    rounding each: EPS (2 w |g - m| + |m_new|) + w dg; u: 2 EPS |ref| + dg (one product, or one
    sum of |g|); p: 4 EPS (|p| + |update|) plus clr bound_m / u + |update| bound_u / u."""
    p, g, m, u = p.to(ACC), g.to(ACC), m.to(ACC), u.to(ACC)
    fb1, fb2, feps, fwd = f32(b1), f32(b2), f32(eps), f32(wd)
    gr = g + fwd * p
    w1 = 1.0 - fb1
    mn = m + w1 * (gr - m)
    un = torch.maximum(u * fb2, gr.abs() + feps)
    clr = lr / (1.0 - b1 ** step)
    upd = clr * mn / un
    dg = EPS * (gr.abs() + (fwd * p).abs()) if fwd != 0.0 else torch.zeros_like(gr)
    bound_m = EPS * (2 * w1 * (gr - m).abs() + mn.abs()) + w1 * dg
    bound_u = 2 * EPS * un + dg
    bound_p = 4 * EPS * (p.abs() + upd.abs()) + clr * bound_m / un + upd.abs() * bound_u / un
    return _ns(p=p - upd, m=mn, u=un, bound_p=bound_p, bound_m=bound_m, bound_u=bound_u)
