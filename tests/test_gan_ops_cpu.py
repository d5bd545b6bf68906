"""CPU checks around the GAN-side ops: the BatchNorm partial workspace of a compiled plan covers
what every BatchNorm descriptor's forward and backward touch (dvie_bn_partial_doubles), the
argument validation of dvie_bn_* / dvie_sn_fwd / dvie_head_bwd (it returns before any launch),
and the fp64 references of tests/gan_ref.py against torch.nn.functional, autograd and the
oracle's Adam.  Nothing is launched."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as F

import gan_ref as R
from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import nets
from oracle import disc as OD


# ---------------- plan sizing ----------------
def _local_disc_plan(n, H, W, dtype=torch.float32):
    """FrameLocalDiscriminator: six BatchNorms, at full, half and quarter resolution"""
    torch.manual_seed(3)
    d = nets.FrameLocalDiscriminator(types.SimpleNamespace(seg_disc=True, precision="fp32"))
    return d._build_plan((n, H, W, dtype, True, True, (True, True), True, torch.device("cpu")))


@pytest.mark.parametrize("n,H,W,splits", [(1, 32, 32, 1), (2, 64, 64, 4)])
def test_bn_partial_covers_every_descriptor(n, H, W, splits):
    """(1, 32, 32): every BatchNorm has fewer than 4096 rows, so one split each, and the
    backward's four coefficient rows are the larger need; (2, 64, 64): the first BatchNorm has
    8192 rows.  [partial, partial + 8 * dvie_bn_partial_doubles(d)) of every BatchNorm
    descriptor lies inside the plan's bn_partial."""
    lib = L.load()
    plan = _local_disc_plan(n, H, W)
    assert plan.bn_splits == splits
    lo = plan.bn_partial.data_ptr()
    hi = lo + plan.bn_partial.numel() * plan.bn_partial.element_size()
    assert plan.bn_partial.dtype == torch.float64
    seen = {L.OP_BN_FWD: 0, L.OP_BN_BWD: 0}
    rows = []
    for ops in (plan.fwd, plan.bwd):
        for o in ops:
            if o.kind not in seen:
                continue
            d = o.u.bn
            seen[o.kind] += 1
            rows.append(d.rows)
            need = lib.dvie_bn_partial_doubles(ctypes.byref(d))
            assert d.splits == lib.dvie_bn_partial_splits(ctypes.byref(d))
            assert need == max(d.splits * 2 * d.c, 4 * d.c)
            assert lo <= d.partial and d.partial + 8 * need <= hi, (d.rows, d.c, d.splits, need, hi - lo)
    assert seen[L.OP_BN_FWD] == 6 and seen[L.OP_BN_BWD] == 6
    assert (max(rows) < 4096) == (splits == 1)


def test_bn_partial_doubles_query():
    lib = L.load()
    d = L.BnDesc()
    for rows, c, want in ((1, 4, 16), (37, 64, 256), (4095, 1024, 4096), (4096, 8, 32), (6145, 12, 72),
                          (2048 * 600, 4, 512 * 2 * 4)):
        d.rows, d.c = rows, c
        assert lib.dvie_bn_partial_doubles(ctypes.byref(d)) == want, (rows, c)
    assert lib.dvie_bn_partial_doubles(None) == 0


# ---------------- argument validation ----------------
def _refused(rc, *words):
    assert rc == L.DVIE_EINVAL
    msg = L.load().dvie_last_error().decode()
    assert all(w in msg for w in words), msg


def _bn_desc(c, x_ld):
    buf = (ctypes.c_float * 16)()
    d = L.BnDesc()
    d.x = d.y = d.g = d.dx = d.stats = d.partial = ctypes.addressof(buf)
    d.rows, d.c, d.splits, d.training = 2, c, 1, 1
    d.x_ld = d.y_ld = d.g_ld = d.dx_ld = x_ld
    d.dtype = L.F32
    return d, buf


@pytest.mark.parametrize("c,x_ld,word", [(6, 8, "multiple of 4"), (1028, 1028, "multiple of 4"), (8, 4, "x_ld")])
def test_bn_refuses_bad_shapes(c, x_ld, word):
    lib = L.load()
    d, _buf = _bn_desc(c, x_ld)
    _refused(lib.dvie_bn_fwd(ctypes.byref(d), None), "bn", word)
    _refused(lib.dvie_bn_bwd(ctypes.byref(d), None), "bn", word)


def _sn_layer(h, width):
    buf = (ctypes.c_float * 4)()
    a = (L.SnLayer * 1)()
    a[0].w_bar = a[0].u = a[0].v = a[0].w_eff = ctypes.addressof(buf)
    a[0].h, a[0].width, a[0].power_iterations = h, width, 1
    return a, buf


def test_sn_refuses_what_its_launch_cannot_allocate():
    """The kernels keep v (width), u (h) and W v (h) in LDS: (width + 2 h) floats, at most 64 KiB.
    h = 16000, width = 8 needs 128032 bytes (the old check bounded h + 2 width and let it
    through to a failing launch); its mirror h = 8, width = 16000 needs 64064 and fits, so only
    the shapes around the limit are probed on the refusing side."""
    lib = L.load()
    for h, width in ((16000, 8), (8192, 1), (1, 16383), (5000, 6385)):
        assert (width + 2 * h) * 4 > 65536
        a, buf = _sn_layer(h, width)
        _refused(lib.dvie_sn_fwd(ctypes.addressof(a), 1, ctypes.addressof(buf), None), "sn layer 0", "LDS")
    assert (16000 + 2 * 8) * 4 <= 65536


def test_head_bwd_refuses_c_not_multiple_of_4():
    buf = (ctypes.c_float * 16)()
    d = L.HeadDesc()
    d.gx = d.gout = ctypes.addressof(buf)
    d.n, d.h, d.w, d.c, d.pool, d.gx_ld = 1, 2, 2, 6, 1, 8
    _refused(L.load().dvie_head_bwd(ctypes.byref(d), None), "head bwd")


# ---------------- the references against torch ----------------
BN_SHAPES = [(2, 4), (37, 12), (2049, 64), (4097, 12), (6145, 4), (37, 1024)]


@pytest.mark.parametrize("rows,c", BN_SHAPES)
@pytest.mark.parametrize("affine,lrelu", [(True, True), (False, False)])
def test_ref_bn_matches_torch(rows, c, affine, lrelu):
    """momentum, eps and alpha that fp32 holds exactly, so gan_ref's float constants are torch's"""
    gen = torch.Generator().manual_seed(rows + c)
    x = (torch.randn((rows, c), generator=gen, dtype=torch.float64) * 2 + 3).requires_grad_(True)
    gamma = (0.5 + torch.rand(c, generator=gen, dtype=torch.float64)).requires_grad_(affine)
    beta = torch.randn(c, generator=gen, dtype=torch.float64).requires_grad_(affine)
    rm, rv = torch.randn(c, generator=gen, dtype=torch.float64), 0.5 + torch.rand(c, generator=gen, dtype=torch.float64)
    gy = torch.randn((rows, c), generator=gen, dtype=torch.float64)
    mom, eps, alpha = 0.125, 2.0 ** -16, 0.25
    trm, trv = rm.clone(), rv.clone()
    pre = F.batch_norm(x, trm, trv, gamma if affine else None, beta if affine else None, True, mom, eps)
    y = F.leaky_relu(pre, alpha) if lrelu else pre
    ref = R.bn_fwd(x.detach(), gamma.detach() if affine else None, beta.detach() if affine else None, rm, rv,
                   momentum=mom, eps=eps, lrelu=lrelu, alpha=alpha)
    assert float((ref.y - y.detach()).abs().max()) < 1e-12 * max(1.0, float(y.detach().abs().max()))
    assert float((ref.running_mean - trm).abs().max()) < 1e-12 and float((ref.running_var - trv).abs().max()) < 1e-12
    pre.backward(gy)  # the kernel's g is the gradient of the pre-activation output
    rb = R.bn_bwd(x.detach(), gy, gamma.detach() if affine else None, ref.mean, ref.invstd)
    scale = max(1.0, float(x.grad.abs().max()))
    assert float((rb.dx - x.grad).abs().max()) < 1e-12 * scale
    if affine:
        assert float((rb.dgamma - gamma.grad).abs().max()) < 1e-12 * max(1.0, float(gamma.grad.abs().max()))
        assert float((rb.dbeta - beta.grad).abs().max()) < 1e-12 * max(1.0, float(beta.grad.abs().max()))
    # eval mode
    ye = F.batch_norm(x.detach(), rm, rv, gamma.detach() if affine else None, beta.detach() if affine else None,
                      False, mom, eps)
    re = R.bn_fwd(x.detach(), gamma.detach() if affine else None, beta.detach() if affine else None, rm, rv,
                  training=False, eps=eps)
    assert float((re.y - ye).abs().max()) < 1e-12 * max(1.0, float(ye.abs().max()))
    assert re.running_mean is None
    for b in (ref.bound_y, rb.bound_dx, rb.bound_dgamma):
        assert bool((b >= 0).all()) and bool(torch.isfinite(b).all())


@pytest.mark.parametrize("n,h,w,c,pool", [(2, 4, 4, 8, 4), (2, 7, 10, 8, 3), (1, 8, 8, 12, 2), (3, 5, 6, 4, 1)])
def test_ref_head_matches_torch(n, h, w, c, pool):
    gen = torch.Generator().manual_seed(h * w)
    x = torch.randn((n, c, h, w), generator=gen, dtype=torch.float64).requires_grad_(True)
    out = F.avg_pool2d(x, pool).reshape(-1, c).mean(1)
    gout = torch.randn(out.shape, generator=gen, dtype=torch.float64)
    out.backward(gout)
    ref = R.head_fwd(x.detach().permute(0, 2, 3, 1), pool)
    assert float((ref.out - out.detach()).abs().max()) < 1e-12
    rb = R.head_bwd(gout, n, h, w, c, pool)
    assert float((rb.gx - x.grad.permute(0, 2, 3, 1)).abs().max()) < 1e-12
    hp, wp = h // pool, w // pool
    assert bool((rb.gx[:, hp * pool:] == 0).all()) and bool((rb.gx[:, :, wp * pool:] == 0).all())


@pytest.mark.parametrize("c", [1, 20])
def test_ref_softmax_matches_torch(c):
    gen = torch.Generator().manual_seed(c)
    x = (torch.rand((2, c, 9, 31), generator=gen, dtype=torch.float64) * 12)
    x[:, 0] += 68 * torch.rand((2, 9, 31), generator=gen, dtype=torch.float64)
    x.requires_grad_(True)
    y = torch.softmax(x, 1)
    gy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(gy)
    ref = R.softmax_fwd(x.detach())
    assert float((ref.y - y.detach()).abs().max()) < 1e-12
    assert float(ref.factor.max()) <= (c + 8 + 80) * R.EPS
    rb = R.softmax_bwd(ref.y, gy, ref.factor)
    assert float((rb.gx - x.grad).abs().max()) < 1e-12


def test_ref_sn_matches_autograd():
    """sigma as a function of (w, u, v) held fixed: gan_ref.sn_bwd is autograd's gradient of
    sum(g_eff * w / sigma)"""
    gen = torch.Generator().manual_seed(9)
    w = torch.randn((5, 7), generator=gen, dtype=torch.float64)
    u0, v0 = torch.randn(5, generator=gen, dtype=torch.float64), torch.randn(7, generator=gen, dtype=torch.float64)
    f = R.sn_fwd(w, u0, v0, 3)
    assert abs(float(f.u.norm()) - 1) < 1e-12 and abs(float(f.v.norm()) - 1) < 1e-12
    sv = torch.linalg.svdvals(w)
    assert float(f.sigma) <= float(sv[0]) * (1 + 1e-12)
    assert R.sn_fwd(w, u0, v0, 0).sigma == u0.dot(w @ v0)
    wa, ua, va = (t.clone().requires_grad_(True) for t in (w, f.u, f.v))
    g_eff = torch.randn((5, 7), generator=gen, dtype=torch.float64)
    (g_eff * (wa / ua.dot(wa.mv(va)))).sum().backward()
    rb = R.sn_bwd(w, g_eff, f.sigma, f.u, f.v)
    assert float((rb.g_bar - wa.grad).abs().max()) < 1e-12
    assert float((rb.g_u - ua.grad).abs().max()) < 1e-12 and float((rb.g_v - va.grad).abs().max()) < 1e-12


def test_ref_adam_matches_oracle():
    """betas and eps that fp32 holds exactly (gan_ref applies them as the kernel's floats)"""
    gen = torch.Generator().manual_seed(2)
    p = torch.randn(300, generator=gen, dtype=torch.float64)
    betas, eps, lr = (0.875, 1.0 - 2.0 ** -9), 2.0 ** -27, 1e-3
    P, st = {0: p}, None
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    mine = p
    for step in (1, 2, 3):
        g = torch.randn(300, generator=gen, dtype=torch.float64)
        P, st = OD.adam_101(P, {0: g}, lr, st, betas=betas, eps=eps)
        r = R.adam(mine, g, m, v, step, lr, betas[0], betas[1], eps)
        mine, m, v = r.p, r.m, r.v
        assert float((mine - P[0]).abs().max()) < 1e-12
        assert float((m - st[0]["m"]).abs().max()) < 1e-12 and float((v - st[0]["v"]).abs().max()) < 1e-12


def test_ref_adamax_matches_torch():
    gen = torch.Generator().manual_seed(4)
    p = torch.randn(300, generator=gen, dtype=torch.float64)
    b1, b2, eps, lr = 0.875, 1.0 - 2.0 ** -9, 2.0 ** -27, 2e-3
    tp = p.clone().requires_grad_(True)
    opt = torch.optim.Adamax([tp], lr=lr, betas=(b1, b2), eps=eps)
    m, u = torch.zeros_like(p), torch.zeros_like(p)
    mine = p
    for step in (1, 2, 3):
        g = torch.randn(300, generator=gen, dtype=torch.float64)
        tp.grad = g.clone()
        opt.step()
        r = R.adamax(mine, g, m, u, step, lr, b1, b2, eps)
        mine, m, u = r.p, r.m, r.u
        assert float((mine - tp.detach()).abs().max()) < 1e-12
