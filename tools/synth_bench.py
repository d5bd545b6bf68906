"""Measurements of the video-synthesis path (DESIGN.md "Device-resident video synthesis"):

* arena vs unaliased bytes of the forward-only HRNet plan (computed, nothing allocated);
* achieved GB/s of dvie_synth_finish / dvie_synth_load at 8x256x512;
* frames/s of VideoSynthesizer.extrapolate, eager and graph=True, against the same rollout
  through InterTrainer.mini_test's glue path, at batch 1 and batch 8, 256x512 bf16.  The three
  run alternating in one process after a warm-up, each leg over at least --seconds of work with
  a device synchronisation around it;
* new frames/s of VideoSynthesizer.interpolate on one video, its pairs batched 8 per forward
  against one per forward.

    python tools/synth_bench.py [--seconds 1.0] [--steps 8] [--json out.json]
"""
import argparse
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_video_interpolation_extrapolation_amd import engine as E  # noqa: E402
from deep_video_interpolation_extrapolation_amd import nets  # noqa: E402
from deep_video_interpolation_extrapolation_amd.runners.InterTrainer import InterTrainer  # noqa: E402
from deep_video_interpolation_extrapolation_amd.synth import VideoSynthesizer, synth_finish, synth_load  # noqa: E402


def make_net(large=False):
    a = types.SimpleNamespace(syn_type="extra", highres_large=large, coarse_model="HRNet", precision="bf16")
    torch.manual_seed(1024)
    return nets.ExtraNet(a)


def arena_numbers():
    out = {}
    for large, n, H, W in ((False, 8, 256, 512), (True, 8, 256, 512), (False, 1, 1024, 2048)):
        g = make_net(large).coarse_model._lower(E.Graph(torch.bfloat16), H, W, dry=True, labels=True)
        _, arena, unaliased = E.arena_layout(g, n)
        out[f"{'large ' if large else ''}{n}x{H}x{W}"] = dict(arena_bytes=arena, unaliased_bytes=unaliased,
                                                              arena_gib=arena / 2 ** 30, unaliased_gib=unaliased / 2 ** 30)
    return out


def timed(fn, seconds):
    """calls per second of fn over at least `seconds` of synchronised work"""
    n, t = 1, 0.0
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        if t >= seconds:
            return n / t
        n = max(n + 1, int(n * min(10.0, 1.2 * seconds / max(t, 1e-4))))


def kernel_numbers(dev, seconds):
    """us per launch and GB/s of algorithmic bytes: on one set of buffers (138 MB / 37 MB, which
    the 256 MiB Infinity Cache holds between launches) and rotating over `sets` of them (more
    than the cache holds, so every launch streams from HBM)"""
    n, H, W = 8, 256, 512
    npix = n * H * W
    out = {}
    for tag, sets in (("cached", 1), ("hbm", 16)):
        rgb = [torch.rand((n, H, W, 8), device=dev) * 2.4 - 1.2 for _ in range(sets)]
        seg = [torch.randn((n, H, W, 24), device=dev) for _ in range(sets)]
        frame = [torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(sets)]
        label = [torch.empty((n, H, W), dtype=torch.uint8, device=dev) for _ in range(sets)]
        u8 = [torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(sets)]
        res = [torch.empty((n, H, W, 8), device=dev) for _ in range(sets)]
        k = [0]

        def fin():
            i = k[0] = (k[0] + 1) % sets
            synth_finish(rgb[i], seg[i], frame[i], label[i])

        def load():
            i = k[0] = (k[0] + 1) % sets
            synth_load(u8[i], res[i])

        r_fin, r_load = timed(fin, seconds), timed(load, seconds)
        out[tag] = dict(buffer_sets=sets, finish_us=1e6 / r_fin, finish_gbs=npix * (128 + 4) * r_fin / 1e9,
                        load_us=1e6 / r_load, load_gbs=npix * (3 + 32) * r_load / 1e9)
    return out


def rollout_numbers(dev, seconds, steps):
    net = make_net().to(dev).eval()
    tr = InterTrainer.__new__(InterTrainer)  # mini_test needs only these
    tr.model, tr.device = net, dev
    tr.args = types.SimpleNamespace(num_pred_once=1, num_pred_step=steps)
    out = {}
    for B in (1, 8):
        H, W = 256, 512
        frames = torch.randint(0, 256, (B, 2, H, W, 3), dtype=torch.uint8, device=dev)
        labels = torch.randint(0, 20, (B, 2, H, W), dtype=torch.uint8, device=dev)
        imgs = [frames[:, t].permute(0, 3, 1, 2).float() / 255 for t in range(2)]
        labs = [labels[:, t].long() for t in range(2)]
        eager, graphed = VideoSynthesizer(net, max_batch=B), VideoSynthesizer(net, max_batch=B, graph=True)
        legs = dict(mini_test=lambda: tr.mini_test(imgs, labs), eager=lambda: eager.extrapolate(frames, labels, steps),
                    graph=lambda: graphed.extrapolate(frames, labels, steps))
        for fn in legs.values():  # warm-up: plans, graph capture
            fn()
            fn()
        rates = {k: [] for k in legs}
        for _ in range(3):  # alternating
            for k, fn in legs.items():
                rates[k].append(timed(fn, seconds) * B * steps)
        out[f"batch{B}"] = {k: dict(frames_per_s=sorted(v)[1], runs=v) for k, v in rates.items()}
    return out


def interpolate_numbers(dev, seconds):
    """new frames/s of interpolate on ONE 17-frame 256x512 video (16 pairs, levels=1): the pairs
    batched 8 per forward (gathered) against one pair per forward (in place), alternating"""
    net = make_net().to(dev).eval()
    frames = torch.randint(0, 256, (1, 17, 256, 512, 3), dtype=torch.uint8, device=dev)
    labels = torch.randint(0, 20, (1, 17, 256, 512), dtype=torch.uint8, device=dev)
    legs = {f"max_batch{mb}": (lambda syn=VideoSynthesizer(net, max_batch=mb): syn.interpolate(frames, labels, 1))
            for mb in (1, 8)}
    for fn in legs.values():
        fn()
        fn()
    rates = {k: [] for k in legs}
    for _ in range(3):
        for k, fn in legs.items():
            rates[k].append(timed(fn, seconds) * 16)
    return {k: dict(frames_per_s=sorted(v)[1], runs=v) for k, v in rates.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--interpolate-only", action="store_true")
    a = ap.parse_args()
    res = dict(arena=arena_numbers())
    if torch.cuda.is_available():
        dev = torch.device("cuda:0")
        if not a.interpolate_only:
            res["kernels_8x256x512"] = kernel_numbers(dev, a.seconds)
        if not a.kernels_only:
            res["interpolate_1x17x256x512_bf16"] = interpolate_numbers(dev, a.seconds)
        if not (a.kernels_only or a.interpolate_only):
            res["extrapolate_256x512_bf16"] = rollout_numbers(dev, a.seconds, a.steps)
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
