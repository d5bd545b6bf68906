"""Op-level parity of the GAN-side kernels -- dvie_bn_fwd / dvie_bn_bwd, dvie_head_fwd /
dvie_head_bwd, dvie_softmax_fwd / dvie_softmax_bwd, dvie_sn_fwd / dvie_sn_bwd, dvie_adam_dev,
dvie_adamax_dev -- called through ctypes, against the plain fp64 references of tests/gan_ref.py.

Comparison: |got - ref| <= K * bound + (rounding of the stored output), elementwise, with the
bounds and constants of gan_ref (derived from the kernels' roundings, never from their output).
Every test prints `RATIO <output>: max error / tolerance`; DESIGN.md ("GAN-side op tests")
records them.

Memory: every tensor a kernel writes (outputs and workspaces) lives inside a larger allocation
filled with the byte 0xA5, with a 64 KiB guard band before and after it; the pad columns of a
matrix whose leading dimension exceeds its width keep that fill too.  After the launches every
guard band and pad column is compared with the fill, so an out-of-bounds write is a failed
assertion inside memory the test owns.
"""
import ctypes
import math

import pytest
import torch

import gan_ref as R
from deep_video_interpolation_extrapolation_amd import _lib as L

pytestmark = pytest.mark.gpu

GUARD = 1 << 16
FILL = 0xA5
EPS = R.EPS


def _es(dt):
    return torch.empty((), dtype=dt).element_size()


class Guarded:
    """device allocations with guard bands (see the module docstring)"""

    def __init__(self, dev):
        self.dev, self.items, self.pads = dev, [], []

    def alloc(self, shape, dtype, name):
        nbytes = math.prod(shape) * _es(dtype)
        raw = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=self.dev)
        self.items.append((name, raw, nbytes))
        return raw[GUARD:GUARD + nbytes].view(dtype).view(shape)

    def put(self, data, name):
        """guarded device copy of a CPU tensor"""
        t = self.alloc(tuple(data.shape), data.dtype, name)
        t.copy_(data)
        return t

    def mat(self, rows, c, ld, dtype, name, data=None):
        """(rows, ld) matrix; columns [0, c) hold `data` (or the fill), the pad columns the fill"""
        t = self.alloc((rows, ld), dtype, name)
        if data is not None:
            t[:, :c] = data.to(self.dev)
        self.pads.append((name, t, c))
        return t

    def check(self):
        torch.cuda.synchronize()
        for name, raw, nbytes in self.items:
            assert bool((raw[:GUARD] == FILL).all()), f"{name}: write before the tensor"
            assert bool((raw[GUARD + nbytes:] == FILL).all()), f"{name}: write past the tensor"
        for name, t, c in self.pads:
            assert bool((t[:, c:].contiguous().view(torch.uint8) == FILL).all()), f"{name}: write into the pad columns"


def close(label, got, ref, tol):
    """assert |got - ref| <= tol elementwise (tol == 0: exact) and print the largest ratio"""
    got, ref, tol = got.detach().double().cpu().reshape(-1), ref.double().reshape(-1), tol.double().reshape(-1)
    assert got.shape == ref.shape == tol.shape, (label, got.shape, ref.shape, tol.shape)
    assert bool(torch.isfinite(got).all()), f"{label}: non-finite output"
    ratio = float(((got - ref).abs() / tol.clamp_min(1e-300)).max()) if got.numel() else 0.0
    print(f"RATIO {label}: {ratio:.3e}")
    assert ratio <= 1.0, f"{label}: error / tolerance = {ratio:.3e}"
    return ratio


def rel_l2(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / max(1e-300, float(b.norm())))


def call(fn, *args):
    L.check(fn(*args), fn.__name__)
    torch.cuda.synchronize()


def up(t):
    return t.detach().double().cpu()


# ---------------- BatchNorm ----------------
# (affine, lrelu, running statistics, accumulate, beta_dx)
BN_MODES = [
    (True, True, True, False, False),
    (False, False, False, False, True),
    (True, False, True, True, True),
    (True, True, False, True, False),
    (False, True, True, False, False),
]
BN_KINDS = ["f32", "bf16", "bf16_xf32"]
BN_C = [4, 12, 64, 1024]
BN_ROWS = [2, 37, 2049, 4097, 6145]
BN_SPLITS = {2: 1, 37: 1, 2049: 1, 4097: 2, 6145: 3}


def bn_data(rows, c, kind, seed):
    """channel 0: |mean| = 1000 standard deviations; channel 1: exactly constant; the rest ordinary"""
    gen = torch.Generator().manual_seed(seed)
    xdt = torch.bfloat16 if kind == "bf16" else torch.float32
    tdt = torch.float32 if kind == "f32" else torch.bfloat16
    sig = 0.5 + 1.5 * torch.rand(c, generator=gen)
    mu = torch.randn(c, generator=gen)
    sig[0], mu[0] = 0.5, 500.0
    x = torch.randn((rows, c), generator=gen) * sig + mu
    x[:, 1] = 0.75
    d = dict(x=x.to(xdt), g=torch.randn((rows, c), generator=gen).to(tdt),
             gamma=0.5 + torch.rand(c, generator=gen), beta=torch.randn(c, generator=gen),
             rm=torch.randn(c, generator=gen), rv=0.5 + torch.rand(c, generator=gen),
             dx0=torch.randn((rows, c), generator=gen).to(tdt),
             dgamma0=torch.randn(c, generator=gen), dbeta0=torch.randn(c, generator=gen))
    return d, xdt, tdt


def run_bn(dev, rows, c, kind, mode, training=True, seed=0, label=None):
    """forward (+ backward in training mode) of one BatchNorm case; returns the raw outputs"""
    affine, lrelu, running, accumulate, beta_dx = mode
    running = running or not training
    lib = L.load()
    st = L.stream_ptr(dev)
    D, xdt, tdt = bn_data(rows, c, kind, seed)
    label = label or f"bn {kind} c={c} rows={rows}"
    G = Guarded(dev)
    x_ld, y_ld, g_ld, dx_ld = c + 4, c + 8, c + 12, c + 4
    X = G.mat(rows, c, x_ld, xdt, "x", D["x"])
    Y = G.mat(rows, c, y_ld, tdt, "y")
    gam = G.put(D["gamma"], "gamma") if affine else None
    bet = G.put(D["beta"], "beta") if affine else None
    rm = G.put(D["rm"], "running_mean") if running else None
    rv = G.put(D["rv"], "running_var") if running else None
    d = L.BnDesc()
    d.x, d.y, d.x_ld, d.y_ld = X.data_ptr(), Y.data_ptr(), x_ld, y_ld
    d.gamma, d.beta = (gam.data_ptr(), bet.data_ptr()) if affine else (None, None)
    d.running_mean, d.running_var = (rm.data_ptr(), rv.data_ptr()) if running else (None, None)
    d.rows, d.c, d.training = rows, c, int(training)
    d.act, d.alpha, d.eps, d.momentum = (L.ACT_LRELU if lrelu else L.ACT_NONE), 0.2, 1e-5, 0.1
    d.dtype, d.x_f32 = (L.F32 if kind == "f32" else L.BF16), int(kind == "bf16_xf32")
    d.splits = lib.dvie_bn_partial_splits(ctypes.byref(d))
    if rows in BN_SPLITS:
        assert d.splits == BN_SPLITS[rows]
    n_partial = lib.dvie_bn_partial_doubles(ctypes.byref(d))
    assert n_partial == max(d.splits * 2 * c, 4 * c) and GUARD >= 4 * c * 8
    partial = G.alloc((n_partial,), torch.float64, "partial")  # exactly the queried size, then the guard
    stats = G.alloc((8, c), torch.float32, "stats")
    d.partial, d.stats = partial.data_ptr(), stats.data_ptr()

    call(lib.dvie_bn_fwd, ctypes.byref(d), st)
    x64 = up(D["x"])
    gamma, beta = (D["gamma"], D["beta"]) if affine else (None, None)
    ref = R.bn_fwd(x64, gamma, beta, D["rm"] if running else None, D["rv"] if running else None, training=training,
                   momentum=0.1, eps=1e-5, lrelu=lrelu, alpha=0.2)
    se = R.store_eps(tdt)
    close(f"{label} y", Y[:, :c], ref.y, R.K_BN_FWD * ref.bound_y + (se * ref.y.abs() if tdt != torch.float32 else 0))
    close(f"{label} mean", stats[0], ref.mean, 2 * EPS * ref.mean.abs())
    close(f"{label} invstd", stats[1], ref.invstd, 2 * EPS * ref.invstd.abs())
    out = dict(y=Y.clone(), stats=stats[:4].clone())
    if running and training:
        close(f"{label} running_mean", rm, ref.running_mean, 2 * EPS * ref.running_mean.abs())
        close(f"{label} running_var", rv, ref.running_var, 2 * EPS * ref.running_var.abs())
        out.update(rm=rm.clone(), rv=rv.clone())
    elif running:
        assert torch.equal(rm.cpu(), D["rm"]) and torch.equal(rv.cpu(), D["rv"])
    if not training:
        G.check()
        return out

    Gm = G.mat(rows, c, g_ld, tdt, "g", D["g"])
    DX = G.mat(rows, c, dx_ld, tdt, "dx", D["dx0"] if beta_dx else None)
    d.g, d.dx, d.g_ld, d.dx_ld = Gm.data_ptr(), DX.data_ptr(), g_ld, dx_ld
    d.accumulate, d.beta_dx = int(accumulate), int(beta_dx)
    dgam = dbet = None
    if affine:
        dgam = G.put(D["dgamma0"], "dgamma") if accumulate else G.alloc((c,), torch.float32, "dgamma")
        dbet = G.put(D["dbeta0"], "dbeta") if accumulate else G.alloc((c,), torch.float32, "dbeta")
        d.dgamma, d.dbeta = dgam.data_ptr(), dbet.data_ptr()
    call(lib.dvie_bn_bwd, ctypes.byref(d), st)
    rb = R.bn_bwd(x64, up(D["g"]), gamma, ref.mean, ref.invstd)
    tol = R.K_BN_DX * rb.bound_dx
    if beta_dx:  # dx rounded to fp32, added to the prior in fp32, stored
        total = rb.dx + up(D["dx0"])
        tol = tol + EPS * rb.dx.abs() + EPS * total.abs() + (se * total.abs() if tdt != torch.float32 else 0)
    else:
        total = rb.dx
        tol = tol + se * total.abs()
    close(f"{label} dx", DX[:, :c], total, tol)
    out.update(dx=DX.clone())
    if affine:
        tg = rb.dgamma + (D["dgamma0"].double() if accumulate else 0)
        tb = rb.dbeta + (D["dbeta0"].double() if accumulate else 0)
        close(f"{label} dgamma", dgam, tg, R.K_BN_DGAMMA * (rb.bound_dgamma + EPS * tg.abs()))
        close(f"{label} dbeta", dbet, tb, 2 * EPS * tb.abs())
        out.update(dgamma=dgam.clone(), dbeta=dbet.clone())
    G.check()
    return out


@pytest.mark.parametrize("rows", BN_ROWS)
@pytest.mark.parametrize("c", BN_C)
@pytest.mark.parametrize("kind", BN_KINDS)
def test_bn_shapes(dev, kind, c, rows):
    """every channel-group layout (c / 4 dividing 256 or not, one lane per group at 1024) times
    every split count (1, 1, 1, 2, 3 with an uneven last split) times the three element-type
    combinations, the modes rotating over the grid"""
    i = BN_KINDS.index(kind) + BN_C.index(c) + BN_ROWS.index(rows)
    run_bn(dev, rows, c, kind, BN_MODES[i % len(BN_MODES)], seed=100 + i)


@pytest.mark.parametrize("mode", BN_MODES)
@pytest.mark.parametrize("kind", BN_KINDS)
def test_bn_modes_and_workspace(dev, kind, mode):
    """rows = 37, c = 64, splits = 1: every mode combination; the backward's four coefficient
    rows (4 c doubles) need twice the [1][2][c] the statistics use, so a partial workspace sized
    by anything smaller than dvie_bn_partial_doubles fails the guard check here"""
    run_bn(dev, 37, 64, kind, mode, seed=7)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("kind", BN_KINDS)
def test_bn_eval(dev, kind, affine):
    """training = 0: the running statistics normalise and stay as they were"""
    run_bn(dev, 2049, 12, kind, (affine, True, True, False, False), training=False, seed=11)


@pytest.mark.parametrize("kind", BN_KINDS)
def test_bn_single_row(dev, kind):
    """rows = 1 in training mode: variance 0, y = act(beta) within the forward bound, finite;
    running_var stays finite (the kernel uses the biased variance where the unbiased one is 0 / 0)"""
    out = run_bn(dev, 1, 12, kind, (True, True, True, False, False), seed=13, label=f"bn {kind} rows=1")
    assert bool(torch.isfinite(out["rv"]).all()) and bool(torch.isfinite(out["rm"]).all())
    D, _, _ = bn_data(1, 12, kind, 13)
    b = D["beta"].double()
    want = torch.where(b > 0, b, b * R.f32(0.2))
    ref = R.bn_fwd(up(D["x"]), D["gamma"], D["beta"], lrelu=True)
    assert torch.equal(ref.y[0], want)
    se = R.store_eps(out["y"].dtype) if out["y"].dtype != torch.float32 else 0
    close(f"bn {kind} rows=1 y vs act(beta)", out["y"][0, :12], want, R.K_BN_FWD * ref.bound_y[0] + se * want.abs())


def test_bn_deterministic(dev):
    """no atomics: two runs of one multi-split case are bitwise equal"""
    a = run_bn(dev, 4097, 12, "bf16_xf32", BN_MODES[2], seed=5)
    b = run_bn(dev, 4097, 12, "bf16_xf32", BN_MODES[2], seed=5)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


# ---------------- discriminator head ----------------
HEAD_SHAPES = [(2, 4, 4, 8, 4), (2, 7, 10, 8, 3), (1, 8, 8, 12, 2), (3, 5, 6, 4, 1)]


@pytest.mark.parametrize("n,h,w,c,pool", HEAD_SHAPES)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_head(dev, dt, n, h, w, c, pool):
    lib = L.load()
    st = L.stream_ptr(dev)
    gen = torch.Generator().manual_seed(n * 1000 + h * 100 + w * 10 + pool)
    hp, wp = h // pool, w // pool
    label = f"head {'f32' if dt == torch.float32 else 'bf16'} {(n, h, w, c, pool)}"
    x = (torch.randn((n, h, w, c), generator=gen) + 0.5).to(dt)
    G = Guarded(dev)
    x_ld, gx_ld = c + 4, c + 8
    X = G.mat(n * h * w, c, x_ld, dt, "x", x.reshape(-1, c))
    pooled = G.alloc((n * c * hp * wp,), torch.float32, "pooled")
    out = G.alloc((n * hp * wp,), torch.float32, "out")
    d = L.HeadDesc()
    d.x, d.out, d.pooled, d.x_ld = X.data_ptr(), out.data_ptr(), pooled.data_ptr(), x_ld
    d.n, d.h, d.w, d.c, d.pool = n, h, w, c, pool
    d.dtype = L.F32 if dt == torch.float32 else L.BF16
    call(lib.dvie_head_fwd, ctypes.byref(d), st)
    ref = R.head_fwd(up(x), pool)
    close(f"{label} out", out, ref.out, R.K_HEAD * ref.bound)
    G.check()

    se = R.store_eps(dt)
    crop = torch.ones((n, h, w), dtype=torch.bool)
    crop[:, :hp * pool, :wp * pool] = False
    crop = crop.reshape(-1)
    gout = torch.randn(n * hp * wp, generator=gen)
    gout_d = gout.to(dev)
    rb = R.head_bwd(gout, n, h, w, c, pool)
    for beta in (0, 1):
        prior = torch.randn((n * h * w, c), generator=gen).to(dt)
        G = Guarded(dev)
        GX = G.mat(n * h * w, c, gx_ld, dt, "gx", prior if beta else None)
        d.gx, d.gx_ld, d.gout, d.beta = GX.data_ptr(), gx_ld, gout_d.data_ptr(), beta
        call(lib.dvie_head_bwd, ctypes.byref(d), st)
        total = rb.gx.reshape(-1, c) + (up(prior) if beta else 0)
        tol = R.K_HEAD * rb.bound.reshape(-1, c) + se * total.abs() + (EPS * total.abs() if beta else 0)
        close(f"{label} gx beta={beta}", GX[:, :c], total, tol)
        got = GX[:, :c].cpu()
        if beta:  # the cropped rows and columns: unchanged
            assert torch.equal(got[crop].view(torch.uint8), prior[crop].view(torch.uint8))
        else:  # exactly zero
            assert int(crop.sum()) == 0 or bool((got[crop] == 0).all())
        G.check()


# ---------------- channel softmax ----------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc_slice"])
@pytest.mark.parametrize("c", [1, 20])
def test_softmax(dev, c, layout):
    lib = L.load()
    st = L.stream_ptr(dev)
    n, h, w = 2, 9, 31  # 558 pixels: three workgroups, the last one partly idle
    gen = torch.Generator().manual_seed(40 + c)
    x = torch.rand((n, c, h, w), generator=gen) * 12
    x[:, 0] += 68 * torch.rand((n, h, w), generator=gen)  # differences up to 80: exp(-80) is a normal fp32
    label = f"softmax c={c} {layout}"
    G = Guarded(dev)
    d = L.SoftmaxDesc()
    if layout == "nchw":
        X = G.put(x, "x")
        d.x, d.sn, d.sc, d.sh, d.sw = X.data_ptr(), c * h * w, h * w, w, 1
    else:  # channels [2, 2 + c) of an NHWC map of c + 4, the other channels far off
        C = c + 4
        full = torch.full((n, h, w, C), 1000.0)
        full[..., 2:2 + c] = x.permute(0, 2, 3, 1)
        X = G.put(full, "x")
        d.x, d.sn, d.sc, d.sh, d.sw = X.data_ptr() + 2 * 4, h * w * C, 1, w * C, C
    Y = G.alloc((n, c, h, w), torch.float32, "y")
    d.y, d.n, d.c, d.h, d.w = Y.data_ptr(), n, c, h, w
    call(lib.dvie_softmax_fwd, ctypes.byref(d), st)
    ref = R.softmax_fwd(x)
    close(f"{label} y", Y, ref.y, R.K_SOFTMAX * ref.bound)
    if c == 1:
        assert bool((Y == 1).all())
    gy = torch.randn((n, c, h, w), generator=gen)
    GY = gy.to(dev)
    for beta in (0, 1):
        prior = torch.randn((n, c, h, w), generator=gen)
        GX = G.put(prior, f"gx{beta}") if beta else G.alloc((n, c, h, w), torch.float32, f"gx{beta}")
        d.gy, d.gx, d.beta = GY.data_ptr(), GX.data_ptr(), beta
        call(lib.dvie_softmax_bwd, ctypes.byref(d), st)
        rb = R.softmax_bwd(up(Y), gy, ref.factor)  # from the y the kernel read
        total = rb.gx + (prior.double() if beta else 0)
        close(f"{label} gx beta={beta}", GX, total, R.K_SOFTMAX * rb.bound + (EPS * total.abs() if beta else 0))
    G.check()


# ---------------- SpectralNorm ----------------
SN_SHAPES = [(1, 1), (3, 5), (5, 3), (37, 300), (64, 48)]


def test_sn_batch_of_17(dev):
    """17 layers in one call: two launches (16 + 1), each with the LDS of its largest layer;
    shapes, power_iterations in {0, 1, 3}, the g_u / g_v pointers (both, u, v, none) and beta
    rotate over the layers; the saved states sit back to back in one exactly sized buffer"""
    lib = L.load()
    st = L.stream_ptr(dev)
    gen = torch.Generator().manual_seed(17)
    G = Guarded(dev)
    n = 17
    arr = (L.SnLayer * n)()
    lay = []
    off = 0
    for i in range(n):
        h, width = SN_SHAPES[i % 5]
        w = torch.randn((h, width), generator=gen) * 0.3
        u = torch.randn(h, generator=gen)
        v = torch.randn(width, generator=gen)
        u, v = u / u.norm(), v / v.norm()
        its = (0, 1, 3)[i % 3]
        has_u, has_v = ((1, 1), (1, 0), (0, 1), (0, 0))[i % 4]
        beta = (i // 4) % 2
        t = dict(h=h, width=width, w=w, u=u, v=v, its=its, beta=beta, off=off,
                 W=G.put(w, f"w{i}"), U=G.put(u, f"u{i}"), V=G.put(v, f"v{i}"),
                 WEFF=G.alloc((h, width), torch.float32, f"w_eff{i}"),
                 g_eff=torch.randn((h, width), generator=gen),
                 bar0=torch.randn((h, width), generator=gen), gu0=torch.randn(h, generator=gen),
                 gv0=torch.randn(width, generator=gen))
        t["GEFF"] = t["g_eff"].to(dev)
        t["GBAR"] = G.put(t["bar0"], f"g_bar{i}") if beta else G.alloc((h, width), torch.float32, f"g_bar{i}")
        t["GU"] = (G.put(t["gu0"], f"g_u{i}") if beta else G.alloc((h,), torch.float32, f"g_u{i}")) if has_u else None
        t["GV"] = (G.put(t["gv0"], f"g_v{i}") if beta else G.alloc((width,), torch.float32, f"g_v{i}")) if has_v else None
        a = arr[i]
        a.w_bar, a.u, a.v, a.w_eff = t["W"].data_ptr(), t["U"].data_ptr(), t["V"].data_ptr(), t["WEFF"].data_ptr()
        a.g_eff, a.g_bar = t["GEFF"].data_ptr(), t["GBAR"].data_ptr()
        a.g_u = t["GU"].data_ptr() if has_u else None
        a.g_v = t["GV"].data_ptr() if has_v else None
        a.state_off, a.h, a.width, a.power_iterations, a.beta = off, h, width, its, beta
        off += 1 + h + width
        lay.append(t)
    state = G.alloc((off,), torch.float32, "state")
    call(lib.dvie_sn_fwd, ctypes.addressof(arr), n, state.data_ptr(), st)
    S = state.cpu()
    worst = dict(sigma=0.0, u=0.0, v=0.0)
    for i, t in enumerate(lay):
        h, width, o = t["h"], t["width"], t["off"]
        t["sigma"], t["us"], t["vs"] = float(S[o]), S[o + 1:o + 1 + h], S[o + 1 + h:o + 1 + h + width]
        ref = R.sn_fwd(t["w"], t["u"], t["v"], t["its"])
        e = dict(sigma=abs(t["sigma"] - float(ref.sigma)) / abs(float(ref.sigma)), u=rel_l2(t["us"], ref.u),
                 v=rel_l2(t["vs"], ref.v))
        for k in e:
            worst[k] = max(worst[k], e[k])
            assert e[k] < 1e-5, (i, k, e[k])
        # u and v in place = the saved copies; untouched without a power iteration
        assert torch.equal(t["U"].cpu(), t["us"]) and torch.equal(t["V"].cpu(), t["vs"])
        if t["its"] == 0:
            assert torch.equal(t["us"], t["u"]) and torch.equal(t["vs"], t["v"])
        rw = R.sn_weff(t["w"], t["sigma"])
        close(f"sn layer {i} {(h, width)} w_eff", t["WEFF"], rw.w_eff, R.K_SN * rw.bound)
    for k, e in worst.items():
        print(f"RATIO sn {k} rel-L2 / 1e-5: {e / 1e-5:.3e}")
    G.check()

    call(lib.dvie_sn_bwd, ctypes.addressof(arr), n, state.data_ptr(), st)
    for i, t in enumerate(lay):
        rb = R.sn_bwd(t["w"], t["g_eff"], t["sigma"], t["us"], t["vs"])
        for name, T, ref, bound, prior in (("g_bar", t["GBAR"], rb.g_bar, rb.bound_bar, t["bar0"]),
                                           ("g_u", t["GU"], rb.g_u, rb.bound_u, t["gu0"]),
                                           ("g_v", t["GV"], rb.g_v, rb.bound_v, t["gv0"])):
            if T is None:
                continue
            total = ref + (prior.double() if t["beta"] else 0)
            close(f"sn layer {i} {(t['h'], t['width'])} {name} beta={t['beta']}", T, total,
                  R.K_SN * bound + (EPS * total.abs() if t["beta"] else 0))
    assert torch.equal(state.cpu(), S)  # the backward only reads the state
    G.check()


# ---------------- Adam / Adamax ----------------
OPT_N = [1, 255, 16384 * 256 + 3]  # the last: past one pass of the largest grid (grid-stride tail)
OPT_STEPS = [(1, 0.0), (2, 1e-2), (1000, 0.0)]  # (device step, weight decay)


@pytest.mark.parametrize("step,wd", OPT_STEPS)
@pytest.mark.parametrize("n", OPT_N)
@pytest.mark.parametrize("which", ["adam", "adamax"])
def test_optimizer_step(dev, which, n, step, wd):
    lib = L.load()
    st = L.stream_ptr(dev)
    gen = torch.Generator().manual_seed(n % 1000 + step)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 0.1
    first = step == 1  # a first step starts from zero moments
    m = torch.zeros(n) if first else torch.randn(n, generator=gen) * 0.1
    s = torch.zeros(n) if first else torch.rand(n, generator=gen) * (0.01 if which == "adam" else 0.1) + 1e-4
    G = Guarded(dev)
    P, M, S = G.put(p, "p"), G.put(m, "m"), G.put(s, "v")
    Gd = g.to(dev)
    stepd = torch.tensor([float(step)], device=dev)
    fn = lib.dvie_adam_dev if which == "adam" else lib.dvie_adamax_dev
    call(fn, P.data_ptr(), Gd.data_ptr(), M.data_ptr(), S.data_ptr(), n, lr, b1, b2, eps, wd, stepd.data_ptr(), st)
    label = f"{which} n={n} step={step} wd={wd}"
    if which == "adam":
        ref = R.adam(p, g, m, s, step, lr, b1, b2, eps, wd)
        second, bound_second = ref.v, ref.bound_v
    else:
        ref = R.adamax(p, g, m, s, step, lr, b1, b2, eps, wd)
        second, bound_second = ref.u, ref.bound_u
    close(f"{label} p", P, ref.p, R.K_OPT * ref.bound_p)
    close(f"{label} m", M, ref.m, R.K_OPT * ref.bound_m)
    close(f"{label} {'v' if which == 'adam' else 'u'}", S, second, R.K_OPT * bound_second)
    assert torch.equal(Gd.cpu(), g) and float(stepd) == step
    G.check()
