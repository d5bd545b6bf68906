"""Time dvie_conv2d_wgrad on 3x3 HRNet shapes under several per-launch environment settings
(DVIE_WG_REUSE, DVIE_WG_DBG, ...: the switches wgrad_halo.hip reads at every launch), the
settings interleaved within each repeat so that they share the box's state.

    python tools/wgrad_ab.py <repeats> <iters> "<setting>;<setting>;..." [shape-substring]

A setting is NAME=VALUE[,NAME=VALUE...] or "-" (nothing set).  DVIE_TOOL_LIB selects the
library (e.g. a -DDVIE_TIMING_DBG build).  One line per shape and setting: every repeat's us per
launch, then min / median / max.  The first result of each setting is checked against torch
(timing-only ablations print their error but are not judged).
"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from deep_video_interpolation_extrapolation_amd import _lib as L  # noqa: E402

if os.environ.get("DVIE_TOOL_LIB"):
    L.LIB_PATH = os.environ["DVIE_TOOL_LIB"]

SHAPES = [  # name, cin, cout, H, W, batch
    ("64->64 256x512", 64, 64, 256, 512, 8),
    ("128->128 128x256", 128, 128, 128, 256, 8),
    ("256->256 64x128", 256, 256, 64, 128, 8),
    ("448->24 256x512", 448, 24, 256, 512, 8),
]


def main():
    repeats, iters = int(sys.argv[1]), int(sys.argv[2])
    settings = [dict(kv.split("=") for kv in s.split(",")) if s != "-" else {} for s in sys.argv[3].split(";")]
    only = sys.argv[4] if len(sys.argv) > 4 else ""
    names = sorted({k for s in settings for k in s})
    lib = L.load()
    dev = torch.device("cuda:0")
    st = L.stream_ptr()
    print("library", L.LIB_PATH)
    for name, cin, cout, H, W, B in SHAPES:
        if only and not any(o in name for o in only.split("|")):
            continue
        torch.manual_seed(0)
        x = torch.randn(B, H, W, cin, device=dev).to(torch.bfloat16)
        g = (torch.randn(B, H, W, cout, device=dev) * 0.1).to(torch.bfloat16)
        ref = torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (cout, cin, 3, 3),
                                          g.float().permute(0, 3, 1, 2), padding=1)
        d = L.WgradDesc()
        d.g, d.x = g.data_ptr(), x.data_ptr()
        d.g_ld, d.x_ld = cout, cin
        d.n, d.oh, d.ow, d.cout = B, H, W, cout
        d.ih, d.iw, d.c, d.sy, d.sx = H, W, cin, 1, 1
        d.th, d.tw, d.dy0, d.dx0, d.ddy, d.ddx = 3, 3, -1, -1, 1, 1
        d.dtype = L.BF16
        d.splits = lib.dvie_wgrad_splits_hint(ctypes.byref(d))
        slabs = lib.dvie_wgrad_slabs(ctypes.byref(d))
        ws = torch.empty(slabs * cout * 9 * cin, device=dev)
        d.ws = ws.data_ptr()
        dw = torch.zeros(cout, cin, 3, 3, device=dev)
        r = L.WreduceDesc()
        r.ws, r.dw, r.cmap = ws.data_ptr(), dw.data_ptr(), None
        r.splits, r.ws_rows, r.ws_k, r.co_off = slabs, cout, 9 * cin, 0
        r.cout_p, r.cin_p, r.kh_n, r.kw_n, r.c, r.beta = cout, cin, 3, 3, cin, 0

        def apply(s):
            for k in names:
                os.environ.pop(k, None)
            os.environ.update(s)

        times = [[] for _ in settings]
        errs = []
        for s in settings:
            apply(s)
            L.check(lib.dvie_conv2d_wgrad(ctypes.byref(d), ctypes.c_void_p(st)), "wgrad")
            L.check(lib.dvie_wgrad_reduce(ctypes.byref(r), ctypes.c_void_p(st)), "wreduce")
            torch.cuda.synchronize()
            errs.append(float((dw - ref).norm() / ref.norm()))
        for _ in range(repeats):
            for i, s in enumerate(settings):
                apply(s)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                lib.dvie_conv2d_wgrad(ctypes.byref(d), ctypes.c_void_p(st))
                e0.record()
                for _ in range(iters):
                    lib.dvie_conv2d_wgrad(ctypes.byref(d), ctypes.c_void_p(st))
                e1.record()
                torch.cuda.synchronize()
                times[i].append(e0.elapsed_time(e1) / iters * 1e3)
        for s, t, e in zip(settings, times, errs):
            tag = ",".join(f"{k}={v}" for k, v in s.items()) or "-"
            print(f"{name:18s} {tag:32s} us " + " ".join(f"{v:6.1f}" for v in t)
                  + f"  min {min(t):6.1f} med {statistics.median(t):6.1f} max {max(t):6.1f}  rel L2 {e:.1e}", flush=True)
        apply({})


if __name__ == "__main__":
    main()
