"""CPU checks around the loss-op tests: the input builders of tests/loss_ref.py have the
properties the GPU comparisons rely on, the fp32 CPU oracle lies inside every bound of the fp64
reference (and every bound is finite and positive), and the comparison the GPU tests use --
`close()` of test_gpu_gan_ops -- rejects eight deliberately wrong references at the smallest case
shape that can show each.  Nothing is launched."""
import pytest
import torch
import torch.nn.functional as F

import loss_ref as R
from oracle import losses as OL
from test_gpu_gan_ops import close

RAGGED = (2, 3, 17, 23)


def _finite_positive(*tols):
    for t in tols:
        t = torch.as_tensor(t)
        assert bool(torch.isfinite(t).all()) and bool((t > 0).all())


def _rejects(label, got, wrong_ref, tol):
    with pytest.raises(AssertionError, match="error / tolerance"):
        close(f"mutant {label}", got, wrong_ref, tol)


# ---------------- builders ----------------
@pytest.mark.parametrize("shape", [(1, 1, 2, 2), RAGGED, (1, 3, 1, 300)])
def test_grid_images_are_exact(shape):
    a, b = R.grid_pair(shape, 5)
    for t in (a, b):
        assert t.dtype == torch.float32 and torch.equal(t * 64, (t * 64).round()) and float(t.abs().max()) <= 1
    d32, d64 = a - b, a.double() - b.double()
    assert torch.equal(d32.double(), d64)
    if shape[-1] > 1:  # differences of differences, as GDL forms them
        dd32 = (a[..., 1:] - a[..., :-1]) - (b[..., 1:] - b[..., :-1])
        dd64 = (a.double()[..., 1:] - a.double()[..., :-1]) - (b.double()[..., 1:] - b.double()[..., :-1])
        assert torch.equal(dd32.double(), dd64)
        nz = dd64[dd64 != 0].abs()
        assert nz.numel() == 0 or float(nz.min()) >= 1 / 64
    nz = d64[d64 != 0].abs()
    assert nz.numel() == 0 or float(nz.min()) >= 1 / 64


def test_grid_images_hold_exact_ties():
    a, b = R.grid_pair(RAGGED, 1)
    assert int((a == b).sum()) > 0
    dx = (a[..., 1:] - a[..., :-1]) - (b[..., 1:] - b[..., :-1])
    assert int((dx == 0).sum()) > 0
    r = R.l1(a, b)
    assert bool((r.grad[a == b] == 0).all())  # sign(0) = 0 in the reference


def test_strided_views_alias():
    t = R.grid_image(RAGGED, R.gen(2))
    B, C, H, W = RAGGED
    cl = R.channels_last(t)
    assert torch.equal(cl, t) and cl.stride() == (H * W * C, 1, W * C, C)
    view, big = R.interior(t)
    assert torch.equal(view, t) and view.data_ptr() == big[0, 1, 2, 3:].data_ptr()
    assert view.stride() == big.stride() and big.shape == (B, C + 2, H + 4, W + 6)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[:, 1:1 + C, 2:2 + H, 3:3 + W] = False
    assert bool((big[mask] == R.PAD_VALUE).all()) and int(mask.sum()) == big.numel() - t.numel()
    for how in ("dense", "cl", "in"):
        assert torch.equal(R.strided(t, how), t)


def test_special_inputs():
    a, b = R.ssim_flat(RAGGED)
    assert int((a != b).sum()) == RAGGED[0] * RAGGED[1] and float((a - b).max()) == pytest.approx(1 / 64, abs=1e-7)
    p, g = R.ssim_near_degenerate(RAGGED)
    assert float(p.mean()) < 0 < float(g.min())
    t = R.soft_tied_target((2, 20, 9, 13), 3)
    mx = t.max(1, keepdim=True).values
    assert float(((t == mx).sum(1) > 1).float().mean()) > 0.9  # ties at nearly every pixel
    a, b = R.mse_pair((3, 3, 7, 9), 4)
    v = R.mse(a, b).value
    assert len({float(x) for x in v}) == 3
    x = R.mixed_magnitudes(65, 1)
    seq, s64, _ = R.sum_f32(x)
    assert seq != float(x.flip(0).numpy().sum(dtype="float32")) or seq != s64  # order matters


# ---------------- the references against the oracle and torch ----------------
def test_ssim_parts_is_the_oracle():
    a, b = R.grid_pair(RAGGED, 8)
    x = a.double().clone().requires_grad_(True)
    v, sq = R.ssim_parts(x, b.double())
    v.backward()
    v64, g64 = R.ssim(a, b)
    assert abs(float(v.detach() - v64)) < 1e-14
    assert float((x.grad + 2 * x.detach() * sq.grad - g64).abs().max()) < 1e-15


def test_reparam_matches_autograd():
    d = R.reparam_inputs(257, 3)
    mu, lv = d.mu.double().requires_grad_(True), d.logvar.double().requires_grad_(True)
    z = d.eps.double() * torch.exp(0.5 * lv) + mu
    z.backward(d.gz.double())
    r = R.reparam(d.mu, d.logvar, d.eps, d.gz)
    assert float((r.z - z.detach()).abs().max()) < 1e-14
    assert float((r.gmu - mu.grad).abs().max()) == 0 and float((r.glogvar - lv.grad).abs().max()) < 1e-14
    assert float(d.logvar.min()) >= -6 and float(d.logvar.max()) <= 4


def test_cosnhwc_matches_oracle_formula():
    g = R.gen(6)
    a, b = torch.randn((2, 20, 5, 7), generator=g).double(), torch.randn((2, 20, 5, 7), generator=g).double()
    x = a / torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True))
    y = b / torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True))
    want = torch.mean(torch.sum(x * y, dim=1))  # oracle.losses.vgg_cosine, one level
    assert abs(float(R.cosnhwc(a, b, 0.2).value) - R.f32(0.2) * float(want)) < 1e-15
    a[1, :, 2, 3] = 0
    assert torch.isnan(R.cosnhwc(a, b).value)
    assert [R.cos_lanes(c) for c in (1, 3, 20, 64, 96, 512)] == [1, 4, 32, 64, 64, 64]


# ---------------- bound sanity: the fp32 oracle lies inside every bound ----------------
@pytest.mark.parametrize("shape", [(1, 1, 2, 2), RAGGED, (2, 3, 300, 300)])
@pytest.mark.parametrize("kind", ["l1", "gdl"])
def test_fp32_oracle_within_l1_gdl_bounds(kind, shape):
    a, b = R.grid_pair(shape, 11)
    fn, of = (R.l1, OL.l1_loss) if kind == "l1" else (R.gdl, OL.gdl_loss)
    for weight in (1.0, 0.37):
        r = fn(a, b, weight)
        x = a.clone().requires_grad_(True)
        v = of(x, b)
        v.backward()
        want, tol = R.stored(r.value, r.bound)
        close(f"{kind} {shape} value", v, want, tol)
        close(f"{kind} {shape} grad", R.f32(weight) * x.grad, r.grad, r.tol_grad)
        _finite_positive(tol, r.tol_grad[r.grad != 0])
    prior = torch.randn(shape, generator=R.gen(1))
    total, tol = R.accumulated(r.grad, r.tol_grad, prior)
    assert torch.equal(total, r.grad + prior.double()) and bool((tol >= r.tol_grad).all())


def test_fp32_oracle_within_mse_bound():
    a, b = R.mse_pair((3, 3, 7, 9), 4)
    r = R.mse(a, b)
    got = torch.stack([torch.mean((a[i] - b[i]) ** 2) for i in range(3)])  # oracle.losses.psnr's d
    for scale, prior in ((1.0, None), (3.0, torch.tensor([1.0, -2.0, 0.5]))):
        want, tol = R.stored(r.value, r.bound, scale, prior)
        close("mse", got * scale + (prior if prior is not None else 0), want, tol)
        _finite_positive(tol)


@pytest.mark.parametrize("builder", ["grid", "degenerate", "flat"])
@pytest.mark.parametrize("shape", [(1, 1, 5, 7), RAGGED])
def test_ssim_tolerance(builder, shape):
    a, b = {"grid": lambda: R.grid_pair(shape, 12), "degenerate": lambda: R.ssim_near_degenerate(shape),
            "flat": lambda: R.ssim_flat(shape)}[builder]()
    t = R.ssim_tolerance(a, b, 0.37)
    _finite_positive(t.tol_value, t.tol_grad)
    close("ssim value", t.v32, t.value, t.tol_value)
    close("ssim grad", R.f32(0.37) * t.g32, t.grad, t.tol_grad)
    print(f"DIST ssim {builder} {shape}: value {t.dist_value:.3e} (ref {float(t.value):.3e}), "
          f"grad {t.dist_grad:.3e} (max|grad| {t.gmax:.3e})")
    # the tolerance stays a small fraction of what it guards
    assert float(t.tol_value) < 0.1 * float(t.value.abs()) and float(t.tol_grad.max()) < 0.05 * R.f32(0.37) * t.gmax


@pytest.mark.parametrize("target", ["onehot", "soft"])
@pytest.mark.parametrize("shape", [(1, 2, 1, 1), (2, 20, 9, 13), (3, 5, 17, 31)])
def test_fp32_oracle_within_ce_bound(shape, target):
    logits = R.ce_logits(shape, 21)
    tgt = R.onehot_target(shape, 22) if target == "onehot" else R.soft_tied_target(shape, 22)
    r = R.ce(logits, tgt, 0.37)
    x = logits.clone().requires_grad_(True)
    v = OL.seg_ce(x, tgt)
    v.backward()
    want, tol = R.stored(r.value, r.bound)
    close("ce value", v, want, tol)
    # torch's backward is exp(log_softmax): its exponent a - m - log s is rounded twice where the
    # kernel's a - m is rounded once, so the oracle is held to twice the kernel's bound
    close("ce grad", R.f32(0.37) * x.grad, r.grad, 2 * r.tol_grad)
    close("ce grad rows", r.grad.sum(1), torch.zeros_like(r.tol_rowsum), r.tol_rowsum)
    _finite_positive(tol, r.tol_grad, r.tol_rowsum)


def test_metric_and_reparam_bounds_are_finite():
    g = R.gen(30)
    for ch in (1, 3, 20, 64, 96, 512):
        a, b = torch.randn((2, ch, 5, 7), generator=g), torch.randn((2, ch, 5, 7), generator=g)
        r = R.cosnhwc(a, b, 0.2)
        want, tol = R.stored(r.value, r.bound)
        _finite_positive(tol)
        x = a / torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True))
        y = b / torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True))
        close(f"cos ch={ch}", R.f32(0.2) * torch.mean(torch.sum(x * y, dim=1)), want, tol)
        r = R.l1nhwc(a.bfloat16(), b.bfloat16())
        want, tol = R.stored(r.value, r.bound)
        _finite_positive(tol)
        close(f"l1nhwc ch={ch}", (a.bfloat16().float() - b.bfloat16().float()).abs().mean(), want, tol)
    d = R.reparam_inputs(2048, 1)
    r = R.reparam(d.mu, d.logvar, d.eps, d.gz)
    _finite_positive(r.bound_z, r.bound_glv[r.glogvar != 0])
    std = d.logvar.mul(0.5).exp_()
    close("reparam z", d.eps.mul(std).add_(d.mu), r.z, r.bound_z)
    assert float(R.iou(torch.tensor([1, 2, 3]), torch.tensor([1, 2, 4])).tol) == 2.0 ** -24
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(0.75) == 2.0 ** -24 and R.ulp32(0) == 0


# ---------------- mutants: the comparison catches a subtly wrong kernel ----------------
def test_mutant_ssim_replicate_padding():
    """(1, 1, 5, 7): the image is smaller than the window, every pixel sees the padding"""
    a, b = R.grid_pair((1, 1, 5, 7), 12)
    t = R.ssim_tolerance(a, b)
    v, g = R.ssim_mutant(a, b, "replicate")
    _rejects("ssim replicate value", t.v32, v, t.tol_value)
    _rejects("ssim replicate grad", t.g32, g, t.tol_grad)


def test_mutant_ssim_gradient_term_dropped_on_partial_tile_row():
    """(2, 3, 17, 23): row 16 is the one row of the second tile row"""
    a, b = R.grid_pair(RAGGED, 12)
    t = R.ssim_tolerance(a, b)
    v, g = R.ssim_mutant(a, b, "drop_beta_last_row")
    assert float(v) == pytest.approx(float(t.value), abs=1e-15)
    assert float((g[..., :16, :] - t.grad[..., :16, :]).abs().max()) < 1e-15  # only row 16 differs
    assert float((g[..., 16:, :] - t.grad[..., 16:, :]).abs().max()) > 1e-6
    _rejects("ssim dropped term", t.g32, g, t.tol_grad)


def test_mutant_gdl_normalisation():
    """(1, 1, 2, 2): W - 1 = W / 2"""
    for shape in ((1, 1, 2, 2), RAGGED):
        a, b = R.grid_pair(shape, 11)
        r = R.gdl(a, b)
        B, C, H, W = shape
        da, db = a.double(), b.double()
        wrong = (((da[..., 1:] - da[..., :-1]) - (db[..., 1:] - db[..., :-1])).abs().sum() / (B * C * H * W)
                 + ((da[..., 1:, :] - da[..., :-1, :]) - (db[..., 1:, :] - db[..., :-1, :])).abs().sum()
                 / (B * C * (H - 1) * W)) / 2
        want, tol = R.stored(r.value, r.bound)
        assert float(r.value) > 0
        _rejects("gdl B C H W", OL.gdl_loss(a, b), wrong, tol)


def test_mutant_ce_last_maximum():
    shape = (2, 20, 9, 13)
    logits, tgt = R.ce_logits(shape, 21), R.soft_tied_target(shape, 22)
    r, wrong = R.ce(logits, tgt), R.ce(logits, tgt, last_max=True)
    x = logits.clone().requires_grad_(True)
    v = OL.seg_ce(x, tgt)
    v.backward()
    _rejects("ce last max value", v, wrong.value, R.stored(r.value, r.bound)[1])
    _rejects("ce last max grad", x.grad, wrong.grad, r.tol_grad)


def test_mutant_mse_samples_swapped():
    a, b = R.mse_pair((3, 3, 7, 9), 4)
    r = R.mse(a, b)
    got = torch.stack([torch.mean((a[i] - b[i]) ** 2) for i in range(3)])
    _rejects("mse swapped", got, r.value.flip(0), R.stored(r.value, r.bound)[1])


def test_mutant_beta_overwrites():
    a, b = R.grid_pair(RAGGED, 11)
    prior = torch.randn(RAGGED, generator=R.gen(1))
    for r in (R.l1(a, b), R.gdl(a, b)):
        total, tol = R.accumulated(r.grad, r.tol_grad, prior)
        _rejects("beta=1 overwrote", (prior.double() + r.grad).float(), r.grad, tol)
    t = R.ssim_tolerance(a, b)
    total, tol = R.accumulated(t.grad, t.tol_grad, prior)
    _rejects("ssim beta=1 overwrote", (prior.double() + t.g32).float(), t.grad, tol)


def test_mutant_cos_channels_past_64():
    g = R.gen(30)
    a, b = torch.randn((2, 96, 5, 7), generator=g), torch.randn((2, 96, 5, 7), generator=g)
    b = b + 0.5 * a
    r, wrong = R.cosnhwc(a, b, 0.2), R.cosnhwc(a, b, 0.2, ch_limit=64)
    x = a / torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True))
    y = b / torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True))
    _rejects("cos ch<64", R.f32(0.2) * torch.mean(torch.sum(x * y, dim=1)), wrong.value,
             R.stored(r.value, r.bound)[1])


def test_mutant_reparam_half():
    d = R.reparam_inputs(255, 1)
    r, wrong = R.reparam(d.mu, d.logvar, d.eps, d.gz), R.reparam(d.mu, d.logvar, d.eps, d.gz, half=1.0)
    got = d.gz * d.eps * 0.5 * torch.exp(0.5 * d.logvar)
    close("reparam glogvar", got, r.glogvar, r.bound_glv)
    _rejects("reparam glogvar without 1/2", got, wrong.glogvar, r.bound_glv)
