"""Measurements of the video-synthesis path (DESIGN.md "Device-resident video synthesis"):

* arena vs unaliased bytes of the forward-only HRNet plan (computed, nothing allocated);
* achieved GB/s of dvie_synth_finish / dvie_synth_load at 8x256x512;
* frames/s of VideoSynthesizer.extrapolate, eager and graph=True, against the same rollout
  through InterTrainer.mini_test's glue path, at batch 1 and batch 8, 256x512 bf16.  The three
  run alternating in one process after a warm-up, each leg over at least --seconds of work with
  a device synchronisation around it;
* new frames/s of VideoSynthesizer.interpolate on one video, its pairs batched 8 per forward
  against one per forward;
* the two-stage path (--two-stage): arena vs unaliased bytes of the three inference plans,
  dvie_synth_bridge's GB/s for both destination layouts, and frames/s of an ExtraStage3Net
  (bf16, stage3_prop) rollout through VideoSynthesizer, eager and graph=True, against the same
  rollout through the module forward plus torch glue, at 8x256x512 (n_scales 1) and
  1x1024x2048 (n_scales 3).

* held-out scoring (--score): us per call and GB/s of algorithmic bytes (8 B per pixel: two RGB
  frames, two label maps) of synth.frame_scores at 8x256x512 and 1x1024x2048, against the same
  scores composed from the public ops there were before it (torch uint8 -> fp32 NCHW, then
  losses.SSIM, losses.PSNR and losses.IoU, one frame at a time), rotating over buffer sets
  that exceed the 256 MiB Infinity Cache, and next to one batch-8 forward.

* the padded canvas (--pad): us per launch and GB/s of dvie_synth_load_pad / dvie_synth_finish_crop
  against dvie_synth_load / dvie_synth_finish on the same canvas (8x256x512 from 253x509 frames,
  1x1088x1920 from a 1080x1920 frame), rotating over buffer sets that exceed the Infinity Cache,
  the legs alternating, three rounds; and frames/s of one ExtraStage3Net rollout (bf16, n_scales 3)
  of a 1080x1920 clip with pad="replicate" against the aligned path on the same clip padded to
  1088x1920 beforehand, alternating in one process, with the differing bytes of the two results.

* the perceptual score (--vgg): us per call of synth.PerceptualScorer on uint8 frames (a) against
  what there was before it for per-frame values (b: per frame, torch uint8 -> fp32 NCHW / 255, then
  losses.VGGCosineLoss at batch 1) and against that composition at the full batch (c: one batch
  mean only, for context), 8 pairs at 256x512 and 1 pair at 1024x2048, bf16, rotating over buffer
  sets that exceed the Infinity Cache, the legs alternating, three rounds; per-op device times of
  one scoring call (load, convs, poolings, cosine reductions, finalize) from events, with the
  algorithmic GB/s of the load and cosine kernels; arena against one buffer per activation; and
  one batch-8 forward for scale.

* multi-scale SSIM (--msssim): us per call of synth.frame_msssim at 5 scales and at 1 beside
  synth.frame_scores on the same frames (no label maps: the SSIM / squared-error pass), 8 pairs at
  256x512 and 1 pair at 1024x2048, rotating over buffer sets that exceed the Infinity Cache, the
  legs alternating, three rounds, the median, with the ratio to frame_scores (the pyramid holds
  1.33 times the pixels of level 0).

* colour conversion (--yuv): us per launch and TB/s of algorithmic bytes (4.5 B per pixel) of
  synth.yuv_to_rgb and synth.rgb_to_yuv, 4:2:0, at 8x256x512 and 1x1080x1920 (where a call's host
  cost exceeds the kernel's device time) and at 64x256x512 and 32x1080x1920, against the same
  conversion composed from torch ops on the device (slicing, float matrix product, round,
  repeat_interleave / avg_pool), rotating over buffer sets that exceed the Infinity Cache, the legs
  alternating, three rounds, the median and the spread, with the ratio composed / kernel.

* scene cuts (--scene): us per call and TB/s of algorithmic bytes of synth.scene_stats (3 B per pixel
  and frame), of synth.scene_cuts (the same pass, the flags written too) and of synth.cut_fill at
  --synth_levels 2 over the frames of the interpolated clip (one flagged pair, and every pair
  flagged: 2 x 3 slots per pair move), on one clip of 8 frames of 256x512 and on one 17-frame
  1080p window, against the same statistic composed from torch ops on the device (integer luma,
  abs difference and sum, index_add_ histogram), rotating over buffer sets that exceed the
  Infinity Cache, the legs alternating, three rounds, the median and the spread.

* tiled synthesis (--tile): us per call and TB/s of algorithmic bytes (every tile element read once,
  the outputs written) of synth.tile_blend for one 2160x3840 canvas from 4 tiles of 1152x2048 at
  overlap 64, 20 classes, with every output and with the frame and label only, against the same blend
  composed from torch ops on the device (weights precomputed), rotating over two buffer sets of
  1.5 GB each, the legs alternating, three rounds, the median and the spread; one forward of a bf16
  coarse InterNet (random weights) at 1080x1920 untiled against tile=(576, 1024), ms per forward
  alternating and max_memory_allocated of each alone; 2160x3840 tiled (1152x2048): frames/s and peak
  memory, with the host guard's refusal of the untiled form recorded (nothing of it is launched);
  and PSNR / mean absolute difference of the tiled against the untiled uint8 frame at 1080x1920,
  inside and outside the overlap bands (information only).

* the self-ensemble (--ensemble): ms per VideoSynthesizer.interpolate call (one forward of the pairs,
  levels=1, bf16 coarse InterNet, random weights) at 8x256x512 and 1x1080x1920 for ensemble=None,
  "time", "flip" and "time+flip", the legs alternating in one process, three rounds, median and
  range, with the ratio to None; and us per launch and TB/s of dvie_synth_flip and
  dvie_synth_ens_acc alone over buffer sets that exceed the Infinity Cache.

    python tools/synth_bench.py [--seconds 1.0] [--steps 8] [--json out.json]
                                [--two-stage | --score | --pad | --vgg | --msssim | --yuv | --scene | --tile | --ensemble]
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
from deep_video_interpolation_extrapolation_amd import losses  # noqa: E402
from deep_video_interpolation_extrapolation_amd.synth import (VideoSynthesizer, frame_scores, synth_bridge,  # noqa: E402
                                                              frame_msssim, synth_finish, synth_finish_crop,
                                                              synth_load, synth_load_pad, synth_flip, synth_ens_acc)


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


def make_two_stage(n_scales):
    a = types.SimpleNamespace(syn_type="extra", highres_large=False, coarse_model="HRNet", precision="bf16",
                              n_scales=n_scales, stage3_prop=True, refine_model="SRNRefine",
                              stage3_model="MSResAttnRefine")
    torch.manual_seed(1024)
    return nets.ExtraStage3Net(a)


TWO_STAGE_SHAPES = ((8, 256, 512, 1), (1, 1024, 2048, 3))  # (n, H, W, n_scales)


def two_stage_arena_numbers():
    """the three inference plans of an ExtraStage3Net forward (bf16, stage3_prop): arena against
    one buffer per activation (computed, nothing allocated)"""
    out = {}
    for n, H, W, ns in TWO_STAGE_SHAPES:
        net = make_two_stage(ns)
        cm = net.coarse_model
        cm._export_stem = True
        graphs = dict(coarse=cm._lower(E.Graph(torch.bfloat16), H, W, dry=True, labels=True),
                      srn=net.refine_model._lower(E.Graph(torch.bfloat16), H, W, False, infer=True),
                      attention=net.stage3_model._lower(E.Graph(torch.bfloat16), H, W, False, True, infer=True))
        cm._export_stem = False
        row = {}
        for k, g in graphs.items():
            _, arena, unaliased = E.arena_layout(g, n)
            row[k] = dict(arena_gib=arena / 2 ** 30, unaliased_gib=unaliased / 2 ** 30, ratio=arena / unaliased)
        row["sum"] = dict(arena_gib=sum(r["arena_gib"] for r in row.values()),
                          unaliased_gib=sum(r["unaliased_gib"] for r in row.values()))
        out[f"{n}x{H}x{W} n_scales={ns}"] = row
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


def bridge_numbers(dev, seconds):
    """dvie_synth_bridge into bf16 destinations, both layouts (SRNRefine's 40 of 56 channels,
    MSResAttnRefine's 24 of 24): us per launch and GB/s of algorithmic bytes (the 32 + 96 B rows of
    image and logits read, the span written), rotating over enough buffer sets to exceed the
    256 MiB Infinity Cache"""
    out = {}
    for n, H, W in ((8, 256, 512), (1, 1024, 2048)):
        npix, sets = n * H * W, 12
        rgb = [torch.rand((n, H, W, 8), device=dev) * 2.4 - 1.2 for _ in range(sets)]
        seg = [torch.randn((n, H, W, 24), device=dev) for _ in range(sets)]
        row = {}
        for tag, span, ld in (("srn", 40, 56), ("attention", 24, 24)):
            dst = [torch.zeros((n, H, W, ld), dtype=torch.bfloat16, device=dev) for _ in range(sets)]
            k = [0]

            def run():
                i = k[0] = (k[0] + 1) % sets
                synth_bridge(rgb[i], seg[i], dst[i][..., :span])

            r = timed(run, seconds)
            row[tag] = dict(us=1e6 / r, gbs=npix * (128 + 2 * span) * r / 1e9, buffer_sets=sets)
            del dst
        out[f"{n}x{H}x{W}"] = row
    return out


def composed_scores(pred, gt, pl, gl, ssim=losses.SSIM(), psnr=losses.PSNR(), iou=losses.IoU()):
    """the baseline of --score: per frame, uint8 -> fp32 [0, 1] NCHW in torch, then the public
    metric ops (1 - SSIM, PSNR, pixel accuracy; no per-class counts)"""
    out = []
    with torch.no_grad():
        for k in range(pred.shape[0]):
            a = pred[k:k + 1].permute(0, 3, 1, 2).float() / 255
            b = gt[k:k + 1].permute(0, 3, 1, 2).float() / 255
            out.append((ssim(a, b), psnr(a, b), iou(pl[k:k + 1], gl[k:k + 1])))
    return out


def score_numbers(dev, seconds):
    """frame_scores against composed_scores, alternating, three rounds each; plus one batch-8
    forward (extrapolate one step, 8x256x512 bf16, eager) for scale"""
    out = {}
    for n, H, W in ((8, 256, 512), (1, 1024, 2048)):
        npix = n * H * W
        sets = (320 << 20) // (8 * npix) + 1  # 8 B per pixel and set: more than the cache holds
        pred, gt = ([torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(sets)]
                    for _ in range(2))
        pl, gl = ([torch.randint(0, 20, (n, H, W), dtype=torch.uint8, device=dev) for _ in range(sets)] for _ in range(2))
        k = [0]

        def fused():
            i = k[0] = (k[0] + 1) % sets
            frame_scores(pred[i], gt[i], pl[i], gl[i])

        def composed():
            i = k[0] = (k[0] + 1) % sets
            composed_scores(pred[i], gt[i], pl[i], gl[i])

        legs = dict(fused=fused, composed=composed)
        for fn in legs.values():
            fn()
            fn()
        rates = {name: [] for name in legs}
        for _ in range(3):  # alternating
            for name, fn in legs.items():
                rates[name].append(timed(fn, seconds))
        row = {name: dict(us=1e6 / sorted(v)[1], gbs=8 * npix * sorted(v)[1] / 1e9, runs_us=[1e6 / r for r in v],
                          spread=(max(v) - min(v)) / sorted(v)[1]) for name, v in rates.items()}
        row["buffer_sets"] = sets
        row["composed_over_fused"] = row["composed"]["us"] / row["fused"]["us"]
        out[f"{n}x{H}x{W}"] = row
        del pred, gt, pl, gl
        torch.cuda.empty_cache()
    net = make_net().to(dev).eval()
    frames = torch.randint(0, 256, (8, 2, 256, 512, 3), dtype=torch.uint8, device=dev)
    labels = torch.randint(0, 20, (8, 2, 256, 512), dtype=torch.uint8, device=dev)
    syn = VideoSynthesizer(net, max_batch=8)
    fwd = lambda: syn.extrapolate(frames, labels, 1)  # noqa: E731
    fwd()
    fwd()
    us = 1e6 / sorted(timed(fwd, seconds) for _ in range(3))[1]
    out["forward_8x256x512_bf16_us"] = us
    out["fused_8x256x512_over_forward"] = out["8x256x512"]["fused"]["us"] / us
    out["composed_8x256x512_over_forward"] = out["8x256x512"]["composed"]["us"] / us
    return out


def vgg_arena_numbers():
    """the scoring plan of my_vgg in bf16: arena against one buffer per activation (computed,
    nothing allocated)"""
    from deep_video_interpolation_extrapolation_amd.nets.vgg import my_vgg, vgg19_features
    net, out = my_vgg(vgg19_features()), {}
    for n, H, W in ((8, 256, 512), (1, 1024, 2048)):
        g = E.Graph(torch.bfloat16)
        net.lower_score(g, H, W)
        _, arena, unaliased = E.arena_layout(g, 2 * n)
        out[f"{n}x{H}x{W}"] = dict(arena_bytes=arena, unaliased_bytes=unaliased, arena_mib=arena / 2 ** 20,
                                   unaliased_mib=unaliased / 2 ** 20, ratio=arena / unaliased)
    return out


def _vgg_op_times(scorer, pred, gt, reps=5):
    """device time per launch of one scoring call (one chunk), from events around every op of the
    plan run one by one: median over `reps` -> {"load", "conv", "pool", "cosfeat", "finalize"} in us
    and the algorithmic GB/s of the load and cosine kernels"""
    import ctypes
    from deep_video_interpolation_extrapolation_amd import _lib as L
    from deep_video_interpolation_extrapolation_amd import synth as S
    n, H, W, _ = pred.shape
    dev = pred.device
    plan = scorer.net.score_plan(n, H, W, dev)
    lut = scorer._table(dev)
    ws = torch.empty((plan.cosfeat_ws_doubles,), dtype=torch.float64, device=dev)
    out = torch.empty((n,), dtype=torch.float64, device=dev)
    plan.set_cosfeat(ws, out)
    lib, stream = L.load(), L.stream_ptr(dev)
    ops = plan.fwd_arr
    names = {L.OP_CONV: "conv", L.OP_EW: "pool", L.OP_COSFEAT: "cosfeat"}
    acc = {}
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(ops) - plan.fwd_off + 2)]
        ev[0].record()
        S.vgg_load(pred, gt, plan.input_view("vgg_in"), lut)
        ev[1].record()
        for i in range(plan.fwd_off, len(ops)):
            L.check(lib.dvie_run_ops(ctypes.byref(ops[i]), 1, stream), "op")
            ev[i - plan.fwd_off + 2].record()
        torch.cuda.synchronize()
        row = {"load": ev[0].elapsed_time(ev[1]) * 1e3}
        for i in range(plan.fwd_off, len(ops)):
            k = names[ops[i].kind] if i < len(ops) - 1 else "finalize"
            row[k] = row.get(k, 0.0) + ev[i - plan.fwd_off + 1].elapsed_time(ev[i - plan.fwd_off + 2]) * 1e3
        for k, v in row.items():
            acc.setdefault(k, []).append(v)
    us = {k: sorted(v)[len(v) // 2] for k, v in acc.items()}
    es = 2 if scorer.net.dtype == torch.bfloat16 else 4
    load_bytes = 2 * n * H * W * (3 + 8 * es)  # bytes read + the 8-channel pixel written
    cos_bytes = sum(2 * n * (H >> k) * (W >> k) * c * es for k, c in enumerate((64, 128, 256, 512, 512)))
    total = sum(us.values())
    return dict(us=us, total_us=total, load_share=us["load"] / total, cosfeat_share=(us["cosfeat"] + us["finalize"]) / total,
                load_gbs=load_bytes / us["load"] / 1e3, cosfeat_gbs=cos_bytes / us["cosfeat"] / 1e3)


def vgg_numbers(dev, seconds):
    """PerceptualScorer (a) against the per-frame (b) and full-batch (c) compositions of the public
    ops, bf16; per-op times of a scoring call; one batch-8 forward for scale"""
    from deep_video_interpolation_extrapolation_amd.synth import PerceptualScorer
    os.environ["DVIE_PRECISION"] = "bf16"
    scorer = PerceptualScorer(max_batch=8)
    cosine = losses.VGGCosineLoss().to(dev)
    out = {}
    for n, H, W in ((8, 256, 512), (1, 1024, 2048)):
        npix = n * H * W
        sets = (320 << 20) // (6 * npix) + 1  # 6 B per pixel and set: more than the cache holds
        pred, gt = ([torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(sets)]
                    for _ in range(2))
        k = [0]

        def f32(x):
            return x.permute(0, 3, 1, 2).float() / 255

        def a_scorer():
            i = k[0] = (k[0] + 1) % sets
            scorer(pred[i], gt[i])

        def b_per_frame():
            i = k[0] = (k[0] + 1) % sets
            for j in range(n):
                cosine(f32(pred[i][j:j + 1]), f32(gt[i][j:j + 1]), False)

        def c_full_batch():
            i = k[0] = (k[0] + 1) % sets
            cosine(f32(pred[i]), f32(gt[i]), False)

        rates = _alternate(dict(a_scorer=a_scorer, b_per_frame=b_per_frame, c_full_batch=c_full_batch), seconds)
        row = {name: dict(us=1e6 / sorted(v)[1], runs_us=[1e6 / r for r in v], min_us=1e6 / max(v), max_us=1e6 / min(v),
                          spread=(max(v) - min(v)) / sorted(v)[1]) for name, v in rates.items()}
        row["buffer_sets"] = sets
        row["b_over_a"] = row["b_per_frame"]["us"] / row["a_scorer"]["us"]
        row["c_over_a"] = row["c_full_batch"]["us"] / row["a_scorer"]["us"]
        row["ops"] = _vgg_op_times(scorer, pred[0], gt[0])
        out[f"{n}x{H}x{W}"] = row
        del pred, gt
        torch.cuda.empty_cache()
    net = make_net().to(dev).eval()
    frames = torch.randint(0, 256, (8, 2, 256, 512, 3), dtype=torch.uint8, device=dev)
    labels = torch.randint(0, 20, (8, 2, 256, 512), dtype=torch.uint8, device=dev)
    syn = VideoSynthesizer(net, max_batch=8)
    fwd = lambda: syn.extrapolate(frames, labels, 1)  # noqa: E731
    fwd()
    fwd()
    us = 1e6 / sorted(timed(fwd, seconds) for _ in range(3))[1]
    out["forward_8x256x512_bf16_us"] = us
    out["a_8x256x512_over_forward"] = out["8x256x512"]["a_scorer"]["us"] / us
    return out


def _alternate(legs, seconds, scale=1.0, rounds=3):
    """legs {name: fn}, warmed up, then timed alternating `rounds` times -> {name: calls/s * scale per
    round}"""
    for fn in legs.values():
        fn()
        fn()
    rates = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            rates[name].append(timed(fn, seconds) * scale)
    return rates


def msssim_numbers(dev, seconds):
    """frame_msssim at 5 scales and at 1 beside frame_scores (no label maps), alternating, three
    rounds"""
    out = {}
    for n, H, W in ((8, 256, 512), (1, 1024, 2048)):
        npix = n * H * W
        sets = (320 << 20) // (6 * npix) + 1  # 6 B per pixel and set: more than the cache holds
        pred, gt = ([torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(sets)]
                    for _ in range(2))
        k = [0]

        def rot(fn):
            def run():
                i = k[0] = (k[0] + 1) % sets
                fn(pred[i], gt[i])
            return run

        legs = dict(score=rot(frame_scores), msssim_k5=rot(lambda a, b: frame_msssim(a, b, 5)),
                    msssim_k1=rot(lambda a, b: frame_msssim(a, b, 1)))
        rates = _alternate(legs, seconds)
        row = {name: dict(us=1e6 / sorted(v)[1], runs_us=[1e6 / r for r in v], spread=(max(v) - min(v)) / sorted(v)[1])
               for name, v in rates.items()}
        row["buffer_sets"] = sets
        for name in legs:
            if name != "score":
                row[f"{name}_over_score"] = row[name]["us"] / row["score"]["us"]
        out[f"{n}x{H}x{W}"] = row
        del pred, gt
        torch.cuda.empty_cache()
    return out


def composed_yuv_to_rgb(packed, H, W, mat, yo):
    """4:2:0 packed frames -> uint8 RGB with torch ops: what the kernel replaces (float32, so not
    bit-equal to the integer form; timing only)"""
    n = packed.shape[0]
    ch, cw = (H + 1) // 2, (W + 1) // 2
    y = packed[:, :H * W].reshape(n, H, W).float() - yo
    u = packed[:, H * W:H * W + ch * cw].reshape(n, ch, cw).float() - 128.0
    v = packed[:, H * W + ch * cw:].reshape(n, ch, cw).float() - 128.0
    u = u.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]
    v = v.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]
    return (torch.stack([y, u, v], -1) @ mat).round_().clamp_(0, 255).to(torch.uint8)


def composed_rgb_to_yuv(rgb, mat, off):
    """uint8 RGB (n, H, W, 3), H and W even -> 4:2:0 packed frames with torch ops (float32; timing only)"""
    n, H, W, _ = rgb.shape
    yuv = rgb.float() @ mat
    y = (yuv[..., 0] + off).round_().clamp_(0, 255).to(torch.uint8).reshape(n, -1)
    c = torch.nn.functional.avg_pool2d(yuv[..., 1:].permute(0, 3, 1, 2), 2)
    c = (c + 128.0).round_().clamp_(0, 255).to(torch.uint8).reshape(n, -1)
    return torch.cat([y, c], 1)


def yuv_numbers(dev, seconds):
    """yuv_to_rgb / rgb_to_yuv (4:2:0, bt601, limited range) against the torch compositions,
    alternating, three rounds; buffer sets past the Infinity Cache"""
    from deep_video_interpolation_extrapolation_amd.synth import rgb_to_yuv, yuv_tables, yuv_to_rgb
    inv, fwd, yo = yuv_tables("bt601", False)
    IY, IRV, IBU, IGU, IGV = (v / 65536.0 for v in inv)
    m_inv = torch.tensor([[IY, IY, IY], [0.0, -IGU, IBU], [IRV, -IGV, 0.0]], device=dev)
    m_fwd = (torch.tensor(fwd, dtype=torch.float32, device=dev) / 65536.0).reshape(3, 3).t().contiguous()
    out = {}
    # 8x256x512 and 1x1080x1920 take a few microseconds on the device, less than a call costs on the
    # host; 64x256x512 and 32x1080x1920 (the slots of one window) show the kernels' own rate
    for n, H, W in ((8, 256, 512), (1, 1080, 1920), (64, 256, 512), (32, 1080, 1920)):
        npix = n * H * W
        fb = H * W * 3 // 2
        sets = (320 << 20) // (9 * npix // 2) + 1  # 4.5 B per pixel and set: more than the cache holds
        packed = [torch.randint(0, 256, (n, fb), dtype=torch.uint8, device=dev) for _ in range(sets)]
        rgb = [torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(sets)]
        k = [0]

        def rot(fn):
            def run():
                i = k[0] = (k[0] + 1) % sets
                fn(i)
            return run

        legs = dict(yuv2rgb=rot(lambda i: yuv_to_rgb(packed[i], H, W, "C420", out=rgb[i])),
                    rgb2yuv=rot(lambda i: rgb_to_yuv(rgb[i], "C420", "bt601", False, out=packed[i])),
                    yuv2rgb_composed=rot(lambda i: composed_yuv_to_rgb(packed[i], H, W, m_inv, yo)),
                    rgb2yuv_composed=rot(lambda i: composed_rgb_to_yuv(rgb[i], m_fwd, float(yo))))
        rates = _alternate(legs, seconds)
        row = {name: dict(us=1e6 / sorted(v)[1], runs_us=[1e6 / r for r in v], spread=(max(v) - min(v)) / sorted(v)[1],
                          tbs=4.5 * npix * sorted(v)[1] / 1e12) for name, v in rates.items()}
        row["buffer_sets"] = sets
        for name in ("yuv2rgb", "rgb2yuv"):
            row[f"{name}_composed_over_kernel"] = row[name + "_composed"]["us"] / row[name]["us"]
        out[f"{n}x{H}x{W}"] = row
        del packed, rgb
        torch.cuda.empty_cache()
    return out


def composed_scene_stats(frames):
    """scene_stats of uint8 (B, T, H, W, 3) with torch ops: what the kernel replaces (the same integers)"""
    B, T = frames.shape[:2]
    f = frames.to(torch.int32)
    y = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8
    sad = (y[:, 1:] - y[:, :-1]).abs().sum((2, 3))
    idx = ((y >> 3) + 32 * torch.arange(B * T, device=y.device, dtype=torch.int32).view(B, T, 1, 1)).reshape(-1)
    h = torch.zeros((B * T * 32,), dtype=torch.int32, device=y.device).index_add_(0, idx, torch.ones_like(idx))
    h = h.view(B, T, 32).long()
    return sad, (h[:, 1:] - h[:, :-1]).abs().sum(-1)


def scene_numbers(dev, seconds):
    """scene_stats / scene_cuts / cut_fill against the torch composition of the statistic, alternating,
    three rounds; buffer sets past the Infinity Cache"""
    from deep_video_interpolation_extrapolation_amd.synth import cut_fill, scene_cuts, scene_stats
    out = {}
    levels = 2
    for T, H, W in ((8, 256, 512), (17, 1080, 1920)):
        clip_bytes = T * H * W * 3
        sets = (320 << 20) // clip_bytes + 1
        clips = [torch.randint(0, 256, (1, T, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(sets)]
        a, b = scene_stats(clips[0]), composed_scene_stats(clips[0])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        S = ((T - 1) << levels) + 1
        fsets = (320 << 20) // (S * H * W * 3) + 1
        slots = [torch.randint(0, 256, (S, 1, H, W, 3), dtype=torch.uint8, device=dev).transpose(0, 1) for _ in range(fsets)]
        one = torch.zeros((1, T - 1), dtype=torch.bool, device=dev)
        one[0, (T - 1) // 2] = True
        every = torch.ones((1, T - 1), dtype=torch.bool, device=dev)
        k = [0, 0]

        def rot(fn, which=0, n=sets):
            def run():
                i = k[which] = (k[which] + 1) % n
                fn(i)
            return run

        legs = dict(stats=rot(lambda i: scene_stats(clips[i])),
                    cuts=rot(lambda i: scene_cuts(clips[i], 30.0, 0.25)),
                    stats_composed=rot(lambda i: composed_scene_stats(clips[i])),
                    fill_one_cut=rot(lambda i: cut_fill(slots[i], one, levels), 1, fsets),
                    fill_every_pair=rot(lambda i: cut_fill(slots[i], every, levels), 1, fsets))
        rates = _alternate(legs, seconds)
        moved = dict(stats=clip_bytes, cuts=clip_bytes, stats_composed=clip_bytes, fill_one_cut=2 * 3 * H * W * 3,
                     fill_every_pair=2 * 3 * H * W * 3 * (T - 1))
        row = {name: dict(us=1e6 / sorted(v)[1], runs_us=[1e6 / r for r in v], spread=(max(v) - min(v)) / sorted(v)[1],
                          tbs=moved[name] * sorted(v)[1] / 1e12) for name, v in rates.items()}
        row["buffer_sets"], row["fill_buffer_sets"] = sets, fsets
        row["stats_composed_over_kernel"] = row["stats_composed"]["us"] / row["stats"]["us"]
        out[f"1x{T}x{H}x{W}"] = row
        del clips, slots
        torch.cuda.empty_cache()
    return out


def motion_numbers(dev, seconds):
    """block_motion on one 1080p pair at (R, s) = (16, 0), (16, 1), (32, 0), alternating, three rounds;
    buffer sets past the Infinity Cache.  bytes: the frames' own (2 x 3 H W); SAD operations: blocks x
    (2R+1)^2 candidates x 256 absolute differences"""
    from deep_video_interpolation_extrapolation_amd.synth import MotionSearch, block_motion, motion_grid
    H, W = 1080, 1920
    pair_bytes = 2 * H * W * 3
    sets = (320 << 20) // pair_bytes + 1
    pairs = [torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(sets)]
    k = [0]

    def rot(search):
        def run():
            i = k[0] = (k[0] + 1) % sets
            block_motion(pairs[i][1], pairs[i][0], search)
        return run

    configs = {f"R{r}_s{s}": MotionSearch(r, s, 16) for r, s in ((16, 0), (16, 1), (32, 0))}
    rates = _alternate({name: rot(search) for name, search in configs.items()}, seconds)
    out = dict(buffer_sets=sets, pair_bytes=pair_bytes)
    for name, v in rates.items():
        search = configs[name]
        bh, bw = motion_grid(H, W, search.scale)
        diffs = bh * bw * (2 * search.radius + 1) ** 2 * 256
        mid = sorted(v)[1]
        out[name] = dict(us=1e6 / mid, runs_us=[1e6 / r for r in v], spread=(max(v) - min(v)) / mid, blocks=bh * bw,
                         abs_diffs=diffs, tera_diffs_per_s=diffs * mid / 1e12, frame_tbs=pair_bytes * mid / 1e12)
    return out


def make_inter_net():
    a = types.SimpleNamespace(syn_type="inter", highres_large=False, coarse_model="HRNet", precision="bf16")
    torch.manual_seed(1024)
    return nets.InterNet(a)


def _tile_weights(ys, xs, th, tw, ov, dev):
    """fp32 (nt, th, tw): the blend weight of every tile over its own pixels, and (hp, wp) their sum"""
    def axis(s, e, S):
        c = torch.arange(s, s + e, device=dev)
        a = c - s + 1 if s > 0 else torch.full_like(c, ov + 1)
        b = s + e - c if s + e < S else torch.full_like(c, ov + 1)
        return torch.minimum(torch.minimum(a, b), torch.full_like(c, ov + 1)).float()
    hp, wp = ys[-1] + th, xs[-1] + tw
    w = torch.stack([axis(y, th, hp)[:, None] * axis(x, tw, wp)[None, :] for y in ys for x in xs])
    total = torch.zeros((hp, wp), device=dev)
    for t, (y, x) in enumerate((y, x) for y in ys for x in xs):
        total[y:y + th, x:x + tw] += w[t]
    return w, total


def composed_tile_blend(rgb_tiles, seg_tiles, ys, xs, w, total, frame, label, rgb_out, lcan):
    """the blend with torch ops on the device: what the kernel replaces (every pixel goes through
    w * v / w, so single-covered pixels are not bit-equal; timing only)"""
    nt, n, th, tw, _ = rgb_tiles.shape
    hp, wp = total.shape
    acc = torch.zeros((n, hp, wp, 3), device=rgb_tiles.device)
    seg = torch.zeros((n, hp, wp, 20), device=rgb_tiles.device)
    for t, (y, x) in enumerate((y, x) for y in ys for x in xs):
        acc[:, y:y + th, x:x + tw] += w[t][None, :, :, None] * rgb_tiles[t][..., :3]
        seg[:, y:y + th, x:x + tw] += w[t][None, :, :, None] * seg_tiles[t][..., :20]
    acc /= total[None, :, :, None]
    seg /= total[None, :, :, None]
    frame.copy_((acc.clamp(-1, 1) * 127.5 + 127.5).round_())
    lab = seg.argmax(-1)
    label.copy_(lab)
    if lcan is not None:
        lcan.copy_(lab)
    if rgb_out is not None:
        rgb_out[..., :3] = acc
        rgb_out[..., 3:] = 0


def tile_blend_numbers(dev, seconds):
    from deep_video_interpolation_extrapolation_amd.synth import tile_blend, tile_starts
    hp, wp, th, tw, ov, n = 2160, 3840, 1152, 2048, 64, 1
    ys, xs = tile_starts(hp, th, ov, 4)[0], tile_starts(wp, tw, ov, 4)[0]
    nt, sets = len(ys) * len(xs), 2
    rgb = [torch.rand((nt, n, th, tw, 8), device=dev) * 2.4 - 1.2 for _ in range(sets)]
    seg = [torch.randn((nt, n, th, tw, 24), device=dev) for _ in range(sets)]
    u8 = dict(dtype=torch.uint8, device=dev)
    frame = [torch.empty((n, hp, wp, 3), **u8) for _ in range(sets)]
    label = [torch.empty((n, hp, wp), **u8) for _ in range(sets)]
    lcan = [torch.empty((n, hp, wp), **u8) for _ in range(sets)]
    out = [torch.empty((n, hp, wp, 8), device=dev) for _ in range(sets)]
    w, total = _tile_weights(ys, xs, th, tw, ov, dev)
    k = [0]

    def rot(fn):
        def run():
            i = k[0] = (k[0] + 1) % sets
            fn(i)
        return run

    legs = dict(blend_all_outputs=rot(lambda i: tile_blend(rgb[i], seg[i], ys, xs, ov, frame[i], label[i], out[i], lcan[i])),
                blend_frame_label=rot(lambda i: tile_blend(rgb[i], seg[i], ys, xs, ov, frame[i], label[i])),
                composed_all_outputs=rot(lambda i: composed_tile_blend(rgb[i], seg[i], ys, xs, w, total, frame[i], label[i],
                                                                       out[i], lcan[i])))
    # the two forms agree up to the rounding of w * v / w
    tile_blend(rgb[0], seg[0], ys, xs, ov, frame[0], label[0], out[0], lcan[0])
    composed_tile_blend(rgb[0], seg[0], ys, xs, w, total, frame[1], label[1], out[1], lcan[1])
    agree = dict(frame_bytes_differing=int((frame[0] != frame[1]).sum()), labels_differing=int((label[0] != label[1]).sum()),
                 max_abs_rgb=float((out[0] - out[1]).abs().max()))
    cpix, tbytes = n * hp * wp, nt * n * th * tw * 128
    nbytes = dict(blend_all_outputs=tbytes + cpix * (32 + 3 + 1 + 1), blend_frame_label=tbytes + cpix * 4,
                  composed_all_outputs=tbytes + cpix * (32 + 3 + 1 + 1))
    rates = _alternate(legs, seconds)
    row = {name: dict(us=1e6 / sorted(v)[1], runs_us=[1e6 / r for r in v], spread=(max(v) - min(v)) / sorted(v)[1],
                      tbs=nbytes[name] * sorted(v)[1] / 1e12, algorithmic_bytes=nbytes[name]) for name, v in rates.items()}
    row["buffer_sets"], row["tiles"], row["agreement_with_composed"] = sets, [ys, xs, th, tw], agree
    row["composed_over_kernel"] = row["composed_all_outputs"]["us"] / row["blend_all_outputs"]["us"]
    return row


def _peak_of(net, make, run, dev):
    """max_memory_allocated of run(make()) alone (two calls), the net's plans dropped before and after;
    before_gib: what was allocated when it began (the weights, the clip, whatever else is alive)"""
    import gc
    net.coarse_model._pool.clear()
    net.coarse_model.last_plan = None
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    syn = make()
    run(syn)
    run(syn)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev)
    del syn
    net.coarse_model._pool.clear()
    net.coarse_model.last_plan = None
    gc.collect()
    torch.cuda.empty_cache()
    return dict(peak_gib=peak / 2 ** 30, before_gib=base / 2 ** 30, peak_over_before_gib=(peak - base) / 2 ** 30)


def tile_forward_numbers(dev, seconds):
    from deep_video_interpolation_extrapolation_amd.synth import FrameSizeError
    net = make_inter_net().to(dev).eval()
    out = {}
    # ---- 1080x1920: one forward untiled against 4 tiles of 576x1024 ----
    H, W = 1080, 1920
    frames = torch.randint(0, 256, (1, 2, H, W, 3), dtype=torch.uint8, device=dev)
    labels = torch.randint(0, 20, (1, 2, H, W), dtype=torch.uint8, device=dev)
    make = dict(untiled=lambda: VideoSynthesizer(net, max_batch=1), tiled=lambda: VideoSynthesizer(net, max_batch=1,
                                                                                                   tile=(576, 1024)))
    run = lambda syn: syn.interpolate(frames, labels, 1)  # noqa: E731
    row = {name: _peak_of(net, mk, run, dev) for name, mk in make.items()}
    syns = {name: mk() for name, mk in make.items()}
    rates = _alternate({name: (lambda s=s: run(s)) for name, s in syns.items()}, seconds)
    for name, v in rates.items():
        row[name].update(ms_per_forward=1e3 / sorted(v)[1], runs_ms=[1e3 / r for r in v], spread=(max(v) - min(v)) / sorted(v)[1])
    row["tiles"] = syns["tiled"].tiles(H, W)
    row["tiled_over_untiled"] = row["tiled"]["ms_per_forward"] / row["untiled"]["ms_per_forward"]
    # the difference tiling makes (random weights): the synthesised frame, inside and outside the overlap bands
    a, b = run(syns["untiled"])[0][0, 1].float(), run(syns["tiled"])[0][0, 1].float()
    ys, xs, th, tw = syns["tiled"].tile_grid(H, W)
    cover = torch.zeros((H, W), device=dev)
    for y in ys:
        for x in xs:
            cover[y:y + th, x:x + tw] += 1
    diff = {}
    for name, m in (("overlap_bands", cover > 1), ("outside", cover == 1), ("all", cover >= 1)):
        d = (a - b)[m]
        mse = float((d * d).mean())
        diff[name] = dict(pixels=int(m.sum()), mean_abs=float(d.abs().mean()),
                          psnr=float("inf") if mse == 0 else 10 * torch.log10(torch.tensor(255.0 ** 2 / mse)).item())
    row["tiled_vs_untiled_frame"] = dict(weights="random (seed 1024)", **diff)
    out["1x1080x1920_bf16"] = row
    del syns, a, b
    # ---- 2160x3840: tiled only; the untiled form is refused on the host ----
    H, W = 2160, 3840
    frames = torch.randint(0, 256, (1, 2, H, W, 3), dtype=torch.uint8, device=dev)
    labels = torch.randint(0, 20, (1, 2, H, W), dtype=torch.uint8, device=dev)
    try:
        VideoSynthesizer(net, max_batch=1)._check_size(H, W)
        refusal = None
    except FrameSizeError as e:
        refusal = str(e)
    mk = lambda: VideoSynthesizer(net, max_batch=1, tile=(1152, 2048))  # noqa: E731
    row = _peak_of(net, mk, run, dev)
    syn = mk()
    v = _alternate(dict(tiled=lambda: run(syn)), seconds)["tiled"]
    row.update(frames_per_s=sorted(v)[1], runs=v, spread=(max(v) - min(v)) / sorted(v)[1], tiles=syn.tiles(H, W),
               max_pixels=syn.max_pixels, untiled_refusal=refusal)
    out["1x2160x3840_bf16"] = row
    return out


def pad_kernel_numbers(dev, seconds):
    """load_pad / finish_crop against load / finish on the same canvas, rotating over buffer sets of
    more than 2 GB in all (every launch streams from HBM).  GB/s are of algorithmic bytes: finish
    128 + 4 B per canvas pixel; finish_crop 96 B of logits per canvas pixel it reads (all with
    label_canvas, the frame's without), 32 + 4 B per frame pixel and 1 B per label_canvas pixel;
    load 3 + 32 B per canvas pixel; load_pad 4 B per frame pixel read, 32 + 1 B per canvas pixel."""
    out = {}
    for n, H, W, Hp, Wp in ((8, 253, 509, 256, 512), (1, 1080, 1920, 1088, 1920)):
        cpix, fpix = n * Hp * Wp, n * H * W
        sets = -(-(2200 << 20) // (cpix * 132))
        u8c = dict(dtype=torch.uint8, device=dev)
        rgb = [torch.rand((n, Hp, Wp, 8), device=dev) * 2.4 - 1.2 for _ in range(sets)]
        seg = [torch.randn((n, Hp, Wp, 24), device=dev) for _ in range(sets)]
        frame_c = [torch.empty((n, Hp, Wp, 3), **u8c) for _ in range(sets)]
        label_c = [torch.empty((n, Hp, Wp), **u8c) for _ in range(sets)]
        frame = [torch.empty((n, H, W, 3), **u8c) for _ in range(sets)]
        label = [torch.empty((n, H, W), **u8c) for _ in range(sets)]
        in_c = [torch.randint(0, 256, (n, Hp, Wp, 3), **u8c) for _ in range(sets)]
        in_f = [torch.randint(0, 256, (n, H, W, 3), **u8c) for _ in range(sets)]
        in_l = [torch.randint(0, 20, (n, H, W), **u8c) for _ in range(sets)]
        k = [0]

        def rot(fn):
            def run():
                i = k[0] = (k[0] + 1) % sets
                fn(i)
            return run

        legs = dict(finish=rot(lambda i: synth_finish(rgb[i], seg[i], frame_c[i], label_c[i])),
                    finish_crop=rot(lambda i: synth_finish_crop(rgb[i], seg[i], frame[i], label[i])),
                    finish_crop_canvas=rot(lambda i: synth_finish_crop(rgb[i], seg[i], frame[i], label[i], label_c[i])),
                    load=rot(lambda i: synth_load(in_c[i], rgb[i])),
                    load_pad=rot(lambda i: synth_load_pad(in_f[i], in_l[i], rgb[i], label_c[i])),
                    load_pad_frames_only=rot(lambda i: synth_load_pad(in_f[i], None, rgb[i], None)))
        nbytes = dict(finish=cpix * 132, finish_crop=fpix * 132, finish_crop_canvas=cpix * 97 + fpix * 36,
                      load=cpix * 35, load_pad=fpix * 4 + cpix * 33, load_pad_frames_only=fpix * 3 + cpix * 32)
        rates = _alternate(legs, seconds)
        row = {name: dict(us=1e6 / sorted(v)[1], gbs=nbytes[name] * sorted(v)[1] / 1e9, runs_us=[1e6 / r for r in v],
                          spread=(max(v) - min(v)) / sorted(v)[1]) for name, v in rates.items()}
        row["buffer_sets"] = sets
        out[f"{n}x{H}x{W} on {n}x{Hp}x{Wp}"] = row
        del rgb, seg, frame_c, label_c, frame, label, in_c, in_f, in_l, legs
        torch.cuda.empty_cache()
    return out


def pad_rollout_numbers(dev, seconds, steps):
    """one ExtraStage3Net rollout (bf16, n_scales 3: multiples of 16) of a 1080x1920 clip: pad="replicate"
    against the aligned path (pad=None, the path there was before) on the same clip padded to
    1088x1920 with clamped indices beforehand; alternating, three rounds"""
    H, W = 1080, 1920
    net = make_two_stage(3).to(dev).eval()
    frames = torch.randint(0, 256, (1, 2, H, W, 3), dtype=torch.uint8, device=dev)
    labels = torch.randint(0, 20, (1, 2, H, W), dtype=torch.uint8, device=dev)
    padded, aligned = VideoSynthesizer(net, max_batch=1, pad="replicate"), VideoSynthesizer(net, max_batch=1)
    Hp, Wp = padded.canvas(H, W)
    iy, ix = (torch.arange(c, device=dev).clamp(max=s - 1) for c, s in ((Hp, H), (Wp, W)))
    frames_c = frames.index_select(2, iy).index_select(3, ix).contiguous()
    labels_c = labels.index_select(2, iy).index_select(3, ix).contiguous()
    legs = dict(aligned_on_canvas=lambda: aligned.extrapolate(frames_c, labels_c, steps),
                pad_replicate=lambda: padded.extrapolate(frames, labels, steps))
    rates = _alternate(legs, seconds, scale=steps)
    want, got = legs["aligned_on_canvas"](), legs["pad_replicate"]()
    row = {name: dict(frames_per_s=sorted(v)[1], runs=v, spread=(max(v) - min(v)) / sorted(v)[1])
           for name, v in rates.items()}
    row["canvas"] = [Hp, Wp]
    row["differing_bytes_after_crop"] = dict(frames=int((want[0][:, :, :H, :W] != got[0]).sum()),
                                             labels=int((want[1][:, :, :H, :W] != got[1]).sum()))
    row["pad_over_aligned"] = row["pad_replicate"]["frames_per_s"] / row["aligned_on_canvas"]["frames_per_s"]
    return row


def module_rollout(net, frames, labels, steps):
    """the baseline: the rollout through the module forward plus torch glue (one-hot, cat, argmax,
    quantise), everything on the device; the prediction is the last stage's finest image, fed
    back raw.  The two input frames are normalised by dvie_synth_load, once per rollout (torch
    divides by a scalar as a multiplication by its reciprocal, which is not the same bits), so
    that the result can be compared with the synthesiser's"""
    onehot = lambda lab: torch.nn.functional.one_hot(lab.long(), 20).permute(0, 3, 1, 2).float()  # noqa: E731
    out_f, out_l = [], []
    with torch.no_grad():
        i1, i2 = (synth_load(frames[:, t].contiguous(), torch.empty(frames[:, t].shape[:-1] + (8,), device=frames.device))
                  .permute(0, 3, 1, 2)[:, :3] for t in range(2))
        s1, s2 = onehot(labels[:, 0]), onehot(labels[:, 1])
        for _ in range(steps):
            res = net(torch.cat([i1, i2], 1), seg=torch.cat([s1, s2], 1))
            img, lab = res[3][-1], torch.argmax(res[1], dim=1)
            out_f.append((img.clamp(-1, 1) * 127.5 + 127.5).round().to(torch.uint8).permute(0, 2, 3, 1))
            out_l.append(lab.to(torch.uint8))
            i1, i2, s1, s2 = i2, img, s2, onehot(lab)
    return torch.stack(out_f, 1), torch.stack(out_l, 1)


def two_stage_numbers(dev, seconds, steps):
    out = {}
    for B, H, W, ns in TWO_STAGE_SHAPES:
        net = make_two_stage(ns).to(dev).eval()
        frames = torch.randint(0, 256, (B, 2, H, W, 3), dtype=torch.uint8, device=dev)
        labels = torch.randint(0, 20, (B, 2, H, W), dtype=torch.uint8, device=dev)
        eager, graphed = VideoSynthesizer(net, max_batch=B), VideoSynthesizer(net, max_batch=B, graph=True)
        legs = dict(module=lambda: module_rollout(net, frames, labels, steps),
                    eager=lambda: eager.extrapolate(frames, labels, steps),
                    graph=lambda: graphed.extrapolate(frames, labels, steps))
        for fn in legs.values():  # warm-up: plans, graph capture
            fn()
            fn()
        same = [int((a != b).sum()) for a, b in zip(legs["module"](), legs["eager"]())]  # differing bytes
        rates = {k: [] for k in legs}
        for _ in range(3):  # alternating
            for k, fn in legs.items():
                rates[k].append(timed(fn, seconds) * B * steps)
        row = {k: dict(frames_per_s=sorted(v)[1], runs=v) for k, v in rates.items()}
        row["module_vs_eager_differing_bytes"] = dict(frames=same[0], labels=same[1])
        out[f"{B}x{H}x{W} n_scales={ns}"] = row
        graphed.reset()
        del net, eager, graphed, legs
        torch.cuda.empty_cache()
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


ENSEMBLE_SHAPES = ((8, 256, 512), (1, 1080, 1920))  # (clips = pairs per forward, H, W)


def ensemble_numbers(dev, seconds):
    """the self-ensemble: ms per interpolate() call (one forward of n pairs, levels=1, bf16 coarse
    InterNet, random weights; pad="replicate", which 1080x1920 does not need at the coarse net's
    multiple of 4) for ensemble=None,
    "time", "flip" and "time+flip", alternating in one process, three rounds, median (min - max), with
    the ratio to None; and us per launch and TB/s of algorithmic bytes of dvie_synth_flip (one frame
    and its label map, 33 B read and written per pixel) and dvie_synth_ens_acc (a mirrored member
    added and scaled: the 6 live vectors of member and sums, 2 x 96 B, read and 128 B written per pixel) alone, rotating over buffer sets that
    exceed the Infinity Cache"""
    net = make_inter_net().to(dev).eval()
    out = {}
    for n, H, W in ENSEMBLE_SHAPES:
        frames = torch.randint(0, 256, (n, 2, H, W, 3), dtype=torch.uint8, device=dev)
        labels = torch.randint(0, 20, (n, 2, H, W), dtype=torch.uint8, device=dev)
        legs = {}
        for setting in (None, "time", "flip", "time+flip"):
            syn = VideoSynthesizer(net, max_batch=n, pad="replicate", ensemble=setting)
            legs[str(setting).lower()] = lambda syn=syn: syn.interpolate(frames, labels, 1)
        rates = _alternate(legs, seconds)
        row = {k: dict(ms=1e3 / sorted(v)[1], min_ms=1e3 / max(v), max_ms=1e3 / min(v)) for k, v in rates.items()}
        for k in legs:
            row[k]["over_none"] = row[k]["ms"] / row["none"]["ms"]
        Hp, Wp = -(-H // 4) * 4, -(-W // 4) * 4
        npix = n * Hp * Wp
        sets = (320 << 20) // (160 * npix) + 2
        f32 = dict(dtype=torch.float32, device=dev)
        src = [torch.randn((n, Hp, Wp, 8), **f32) for _ in range(sets)]
        lsrc = [torch.randint(0, 20, (n, Hp, Wp), dtype=torch.uint8, device=dev) for _ in range(sets)]
        dst, ldst = torch.empty_like(src[0]), torch.empty_like(lsrc[0])
        seg = [torch.randn((n, Hp, Wp, 24), **f32) for _ in range(sets)]
        acc_r = [torch.randn((n, Hp, Wp, 8), **f32) for _ in range(sets)]
        acc_s = [torch.randn((n, Hp, Wp, 24), **f32) for _ in range(sets)]
        k = [0]

        def flip():
            i = k[0] = (k[0] + 1) % sets
            synth_flip(src[i], lsrc[i], dst, ldst)

        def acc():
            i = k[0] = (k[0] + 1) % sets
            synth_ens_acc(src[i], seg[i], acc_r[i], acc_s[i], flip=True, last_m=2)

        kr = _alternate(dict(flip=flip, ens_acc=acc), seconds)
        for name, nbytes in (("flip", 2 * 33), ("ens_acc", 2 * 96 + 128)):
            v = kr[name]
            row[f"{name}_kernel"] = dict(us=1e6 / sorted(v)[1], min_us=1e6 / max(v), max_us=1e6 / min(v),
                                         tb_per_s=npix * nbytes * sorted(v)[1] / 1e12, buffer_sets=sets)
        row["scratch_bytes"] = npix * (2 * 32 + 2 + 128)
        out[f"{n}x{H}x{W}"] = row
        del src, lsrc, seg, acc_r, acc_s, frames, labels, legs
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--interpolate-only", action="store_true")
    ap.add_argument("--two-stage", action="store_true", help="only the two-stage legs")
    ap.add_argument("--score", action="store_true", help="only the held-out scoring legs")
    ap.add_argument("--pad", action="store_true", help="only the padded-canvas legs")
    ap.add_argument("--vgg", action="store_true", help="only the perceptual-score legs")
    ap.add_argument("--msssim", action="store_true", help="only the multi-scale SSIM legs")
    ap.add_argument("--yuv", action="store_true", help="only the colour-conversion legs")
    ap.add_argument("--scene", action="store_true", help="only the scene-cut legs")
    ap.add_argument("--tile", action="store_true", help="only the tiled-synthesis legs")
    ap.add_argument("--ensemble", action="store_true", help="only the self-ensemble legs")
    ap.add_argument("--motion", action="store_true", help="only the block-matching legs")
    a = ap.parse_args()
    if a.motion:
        res = dict(motion_1x1080x1920=motion_numbers(torch.device("cuda:0"), a.seconds))
        print(json.dumps(res, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return
    if a.ensemble:
        res = dict(ensemble_interpolate_bf16=ensemble_numbers(torch.device("cuda:0"), a.seconds))
        print(json.dumps(res, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return
    if a.tile:
        dev = torch.device("cuda:0")
        res = dict(tile_blend_2160x3840=tile_blend_numbers(dev, a.seconds))
        torch.cuda.empty_cache()
        res["tile_forward"] = tile_forward_numbers(dev, a.seconds)
        print(json.dumps(res, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return
    if a.scene:
        res = dict(scene=scene_numbers(torch.device("cuda:0"), a.seconds))
        print(json.dumps(res, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return
    if a.yuv:
        res = dict(yuv=yuv_numbers(torch.device("cuda:0"), a.seconds))
        print(json.dumps(res, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return
    if a.msssim:
        res = dict(msssim=msssim_numbers(torch.device("cuda:0"), a.seconds))
        print(json.dumps(res, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return
    if a.vgg:
        res = dict(vgg_arena_bf16=vgg_arena_numbers())
        if torch.cuda.is_available():
            res["vgg_bf16"] = vgg_numbers(torch.device("cuda:0"), a.seconds)
        print(json.dumps(res, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return
    if a.pad:
        dev = torch.device("cuda:0")
        res = dict(pad_kernels=pad_kernel_numbers(dev, a.seconds),
                   pad_rollout_stage3_bf16_1080x1920=pad_rollout_numbers(dev, a.seconds, a.steps))
        print(json.dumps(res, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return
    if a.score:
        res = dict(score=score_numbers(torch.device("cuda:0"), a.seconds))
        print(json.dumps(res, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return
    if a.two_stage:
        res = dict(two_stage_arena=two_stage_arena_numbers())
        if torch.cuda.is_available():
            dev = torch.device("cuda:0")
            res["bridge_bf16"] = bridge_numbers(dev, a.seconds)
            res["extrapolate_stage3_bf16"] = two_stage_numbers(dev, a.seconds, a.steps)
        print(json.dumps(res, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return
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
