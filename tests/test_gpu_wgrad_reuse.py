"""GPU: the 3x3 halo weight gradient's row-walking form (wgrad_halo.hip, REUSE: a wave owns a
column half of the tile and keeps a three-row window of X fragments in registers), through the
C ABI as test_gpu_wgrad.py does -- dvie_conv2d_wgrad into a NaN-filled workspace, then
dvie_wgrad_reduce -- against torch.nn.grad.conv2d_weight in fp64 on the same bf16 operands.

Both sides sum exact bf16 products, the kernel in fp32: relative L2 <= 1e-4 (the project's slab
bar) for the whole gradient AND for each of the 9 taps on its own, so that a wrong (row, tap)
pairing at a border cannot hide in the norm; bias <= 1e-4; everything finite.

Shapes are the smallest that reach each path: one tile with padding above and below; three
tiles of one column in one workgroup (window / ring hand-over); ragged row tile + ragged
16-pixel column + column and image changes inside one range, and a range starting mid-column;
channel padding on both operands with the 4-wave form; 2 x 2 channel blocks; the bias-free
instantiation; the k-step loop (DVIE_WG_REUSE=0) on the same operands.

Also: a th = tw = 2 launch that is no stride-2 phase launch (ws_taps == 0) is the per-tap
kernel's, not the halo kernel's."""
import ctypes
import functools
import os

import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L

pytestmark = pytest.mark.gpu

BAR = 1e-4


@functools.lru_cache(maxsize=None)
def _operands(n, H, W, c, cout):
    """bf16 operands (CPU) and the fp64 references, computed once per shape."""
    gen = torch.Generator().manual_seed(1000 * n + 100 * H + W + c + cout)
    x = torch.randn(n, H, W, c, generator=gen).to(torch.bfloat16)
    g = torch.randn(n, H, W, cout, generator=gen).to(torch.bfloat16)
    xr, gr = x.double().permute(0, 3, 1, 2), g.double().permute(0, 3, 1, 2)
    ref_w = torch.nn.grad.conv2d_weight(xr, (cout, c, 3, 3), gr, padding=1)
    return x, g, ref_w, gr.sum((0, 2, 3))


def _reduce(lib, s, ws_ptr, out, nsl, rows, k, cin):
    r = L.WreduceDesc()
    r.ws, r.dw, r.cmap = ws_ptr, out.data_ptr(), None
    r.splits, r.ws_rows, r.ws_k, r.co_off = nsl, rows, k * k * cin if k > 1 else cin, 0
    r.cout_p, r.cin_p, r.kh_n, r.kw_n, r.c, r.beta = rows, cin, k, k, cin if k > 1 or cin > 1 else 1, 0
    L.check(lib.dvie_wgrad_reduce(ctypes.byref(r), s), "wreduce")


def _run(dev, x, g, th, dy0, splits, bias):
    """dvie_conv2d_wgrad + reductions for a th x th tap grid at offset dy0 = dx0; returns
    (dw, db or None, traced kernel names, splits hint)."""
    lib = L.load()
    n, H, W, c = x.shape
    cout = g.shape[-1]
    xd, gd = x.to(dev), g.to(dev)
    d = L.WgradDesc()
    d.g, d.x = gd.data_ptr(), xd.data_ptr()
    d.g_ld, d.x_ld = cout, c
    d.n, d.oh, d.ow, d.cout = n, H, W, cout
    d.ih, d.iw, d.c, d.sy, d.sx = H, W, c, 1, 1
    d.th, d.tw, d.dy0, d.dx0, d.ddy, d.ddx = th, th, dy0, dy0, 1, 1
    d.dtype = L.BF16
    hint = lib.dvie_wgrad_splits_hint(ctypes.byref(d))
    d.splits = splits if splits else (hint if hint > 0 else 16)
    slabs = lib.dvie_wgrad_slabs(ctypes.byref(d))
    bslabs = 0
    if bias:
        d.bws = 1
        bslabs = lib.dvie_wgrad_bias_slabs(ctypes.byref(d))
    wfl = slabs * cout * th * th * c
    ws = torch.full((wfl + bslabs * cout,), float("nan"), device=dev)
    d.ws = ws.data_ptr()
    d.bws = ws.data_ptr() + 4 * wfl if bias else None
    s = L.stream_ptr(dev)
    lib.dvie_trace_kernels(1)
    L.check(lib.dvie_conv2d_wgrad(ctypes.byref(d), s), "wgrad")
    names = lib.dvie_traced_kernels().decode()
    lib.dvie_trace_kernels(0)
    dw = torch.empty(cout, c, th, th, device=dev)
    _reduce(lib, s, ws.data_ptr(), dw, slabs, cout, th, c)
    db = None
    if bias:
        db = torch.empty(cout, device=dev)
        _reduce(lib, s, ws.data_ptr() + 4 * wfl, db, bslabs, cout, 1, 1)
    torch.cuda.synchronize()
    return dw.cpu().double(), None if db is None else db.cpu().double(), names, hint


def _check(tag, dw, db, ref_w, ref_b):
    ew = float((dw - ref_w).norm() / ref_w.norm())
    taps = [float((dw[:, :, i, j] - ref_w[:, :, i, j]).norm() / ref_w[:, :, i, j].norm())
            for i in range(ref_w.shape[2]) for j in range(ref_w.shape[3])]
    eb = float((db - ref_b).norm() / ref_b.norm()) if db is not None else 0.0
    print(f"{tag}: weight rel L2 {ew:.2e}, per tap " + " ".join(f"{t:.1e}" for t in taps) + f", bias {eb:.2e}")
    assert torch.isfinite(dw).all() and (db is None or torch.isfinite(db).all())
    assert ew <= BAR, ew
    assert max(taps) <= BAR, taps
    assert eb <= BAR, eb


CASES = [  # n, H, W, c, cout, splits (0: the library's hint), bias
    (1, 4, 64, 64, 64, 0, True),       # one tile: padding rows above and below it
    (1, 12, 64, 64, 64, 1, True),      # three tiles of one column in one workgroup
    (2, 10, 80, 64, 64, 1, True),      # ragged row tile, ragged 16-pixel column, column + image changes
    (2, 10, 80, 64, 64, 3, True),      # ... and a range that starts mid-column
    (1, 9, 70, 40, 24, 0, True),       # channel padding on both operands, the 4-wave form
    (1, 8, 64, 128, 128, 0, True),     # 2 x 2 channel blocks
    (1, 12, 64, 64, 64, 1, False),     # no bias pointer (the bias-free instantiation)
]


@pytest.mark.parametrize("case", CASES)
def test_wgrad_reuse_matches_fp64(dev, case):
    n, H, W, c, cout, splits, bias = case
    x, g, ref_w, ref_b = _operands(n, H, W, c, cout)
    dw, db, names, hint = _run(dev, x, g, 3, -1, splits, bias)
    assert hint > 0 and "wgrad_halo_kernel" in names and "wgrad_kernel<" not in names, (hint, names)
    _check(str(case), dw, db, ref_w, ref_b)


def test_wgrad_kstep_loop_same_operands(dev):
    """The k-step loop (DVIE_WG_REUSE=0) on the three-tile case: both loops meet the bar against
    fp64; their mutual difference (fp32 summation order) is printed, not judged."""
    x, g, ref_w, ref_b = _operands(1, 12, 64, 64, 64)
    new_w, new_b, _, _ = _run(dev, x, g, 3, -1, 1, True)
    os.environ["DVIE_WG_REUSE"] = "0"
    old_w, old_b, names, _ = _run(dev, x, g, 3, -1, 1, True)
    assert "wgrad_halo_kernel" in names, names
    print(f"row-walking vs k-step loop: rel L2 {float((new_w - old_w).norm() / old_w.norm()):.2e}")
    _check("k-step loop", old_w, old_b, ref_w, ref_b)
    _check("row-walking loop", new_w, new_b, ref_w, ref_b)


def test_wgrad_2x2_without_shared_slabs_takes_per_tap_kernel(dev):
    """th = tw = 2 at dy0 = dx0 = +1 with ws_taps == 0: only the stride-2 phase launches
    (ws_taps > 0) are tested on the halo kernel's 2 x 2 form, so this one is refused by
    dvie_wgrad_splits_hint and runs on the per-tap kernel."""
    n, H, W, c, cout = 2, 9, 70, 64, 64
    x, g, _, ref_b = _operands(n, H, W, c, cout)
    dw, db, names, hint = _run(dev, x, g, 2, 1, 0, True)
    assert hint == 0, hint
    assert "wgrad_kernel<" in names and "wgrad_halo_kernel" not in names, names
    xp = torch.zeros(n, H + 3, W + 3, c, dtype=torch.float64)
    xp[:, :H, :W] = x.double()
    gd = g.double()
    ref_w = torch.stack([torch.stack([torch.einsum("nyxo,nyxi->oi", gd, xp[:, 1 + i:1 + i + H, 1 + j:1 + j + W])
                                      for j in range(2)], -1) for i in range(2)], -2)
    _check("2x2 per-tap", dw, db, ref_w, ref_b)
