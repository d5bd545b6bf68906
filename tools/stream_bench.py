"""End-to-end wall time and peak device memory of `--split test` (INTER, bf16 coarse net with random
weights, --synth_levels 2) on one synthetic 256x512 clip, three ways, alternating in one process:

  (a) png_whole    the PNG directory, --synth_window 0 (the whole clip at once)
  (b) png_window   the PNG directory, --synth_window W
  (c) y4m_window   the same frames as a C420 Y4M file (Cmono labels), --synth_window W

and, for the memory of a longer clip, a Y4M clip of --long-frames frames with --synth_window W and
with --synth_window 0.  Per run: the wall time of main() (trainer construction, checkpoint load and
plan compilation included; the interpreter start and `import torch` are not), output slots per
second, torch.cuda.max_memory_allocated, and for the windowed runs the per-stage busy and wait times
the command logs.  The clip is smooth moving gradients with mild noise and blocky label maps (PNG
encoding time depends on the content: noise would be slower, flat frames faster).

    python tools/stream_bench.py [--frames 65] [--long-frames 257] [--window 16] [--rounds 3] [--json out.json]

--synth_scd: only leg (c), with and without --synth_scd (default thresholds) in alternation, `--rounds`
times: what detection and the fill launches cost the stream.  The clip has no cuts, so both legs
write the same bytes.
"""
import argparse
import gc
import json
import os
import re
import shutil
import sys
import tempfile
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_video_interpolation_extrapolation_amd import main as M  # noqa: E402
from deep_video_interpolation_extrapolation_amd import nets  # noqa: E402
from deep_video_interpolation_extrapolation_amd.video_io import Y4MWriter  # noqa: E402

H, W = 256, 512


def synthetic_clip(T, seed=0):
    """(frames (T, H, W, 3), labels (T, H, W)) uint8: drifting gradients + noise of +-6, 32x32 label blocks"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    frames = np.empty((T, H, W, 3), dtype=np.uint8)
    labels = np.empty((T, H, W), dtype=np.uint8)
    for t in range(T):
        img = np.stack([127 + 100 * np.sin((x + 3 * t) / 40.0), 127 + 100 * np.cos((y - 2 * t) / 30.0),
                        127 + 100 * np.sin((x + y + t) / 55.0)], -1)
        frames[t] = np.clip(img + rng.randint(-6, 7, img.shape), 0, 255).astype(np.uint8)
        labels[t] = ((x.astype(np.int64) + 2 * t) // 32 + y.astype(np.int64) // 32) % 20
    return frames, labels


def rgb_to_packed_420(frames):
    """host-side BT.601 limited-range 4:2:0 packing of the synthetic frames (float; only to make the input file)"""
    f = frames.astype(np.float32)
    yy = 16 + (65.481 * f[..., 0] + 128.553 * f[..., 1] + 24.966 * f[..., 2]) / 255
    u = 128 + (-37.797 * f[..., 0] - 74.203 * f[..., 1] + 112.0 * f[..., 2]) / 255
    v = 128 + (112.0 * f[..., 0] - 93.786 * f[..., 1] - 18.214 * f[..., 2]) / 255
    T = f.shape[0]
    pool = lambda p: p.reshape(T, H // 2, 2, W // 2, 2).mean(axis=(2, 4))  # noqa: E731
    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8).reshape(T, -1)  # noqa: E731
    return np.concatenate([q(yy), q(pool(u)), q(pool(v))], 1)


def make_data(root, T, png):
    from PIL import Image
    frames, labels = synthetic_clip(T)
    for sub in ("rgb", "seg"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    if png:
        for sub in ("rgb", "seg"):
            os.makedirs(os.path.join(root, sub, "clip"))
        for t in range(T):
            Image.fromarray(frames[t]).save(os.path.join(root, "rgb", "clip", f"{t:04d}.png"))
            Image.fromarray(labels[t]).save(os.path.join(root, "seg", "clip", f"{t:04d}.png"))
    else:
        with Y4MWriter(os.path.join(root, "rgb", "clip.y4m"), W, H, (30, 1), "C420") as w:
            w.write(rgb_to_packed_420(frames))
        with Y4MWriter(os.path.join(root, "seg", "clip.y4m"), W, H, (30, 1), "Cmono") as w:
            w.write(labels.reshape(T, -1))


def run(run_dir, data, window, levels, extra=()):
    """one `--split test` -> dict(wall_s, peak_bytes, stages: the numbers of the command's log line or None)"""
    out = os.path.join(data, "synth")
    shutil.rmtree(out, ignore_errors=True)
    log = os.path.join(run_dir, "experiment_test.log")
    if os.path.exists(log):
        os.remove(log)
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    M.main(["--split", "test", "--syn_type", "inter", "--input_h", str(H), "--input_w", str(W), "--precision", "bf16",
            "--bs", "8", "--load_dir", run_dir, "--checksession", "0", "--checkepoch", "1", "--checkpoint", "0",
            "--cycgen_load_dir", data, "--synth_levels", str(levels), "--synth_window", str(window), *extra, "INTER",
            "--load_coarse"])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated()
    stages = None
    for line in open(log):
        m = re.search(r"synth: \S+ (\d+) slots in ([\d.]+) s .*reader busy ([\d.]+) s, this thread waited for it "
                      r"([\d.]+) s and for the writer ([\d.]+) s, writer busy ([\d.]+) s \(([\d.]+) s after", line)
        if m:
            v = [float(g) for g in m.groups()]
            stages = dict(slots=int(v[0]), clip_s=v[1], reader_busy_s=v[2], waited_for_reader_s=v[3],
                          waited_for_writer_s=v[4], writer_busy_s=v[5], writer_tail_s=v[6])
    shutil.rmtree(out, ignore_errors=True)
    return dict(wall_s=wall, peak_bytes=peak, stages=stages)


def scd_legs(a, run_dir, data):
    """y4m_window without and with --synth_scd, alternating -> median (min - max) wall time of both"""
    legs = dict(scd_off=(), scd_on=("--synth_scd",))
    slots = (a.frames - 1) * (1 << a.levels) + 1
    run(run_dir, data, a.window, a.levels, ("--synth_scd",))  # warm-up: code objects, allocator
    runs = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, extra in legs.items():
            runs[k].append(run(run_dir, data, a.window, a.levels, extra))
    res = {}
    for k, v in runs.items():
        walls = sorted(r["wall_s"] for r in v)
        clip = sorted(r["stages"]["clip_s"] for r in v)
        res[k] = dict(wall_s=walls[len(walls) // 2], wall_min_s=walls[0], wall_max_s=walls[-1],
                      runs_wall_s=[r["wall_s"] for r in v], clip_s=clip[len(clip) // 2], clip_min_s=clip[0],
                      clip_max_s=clip[-1], slots=slots, peak_mib=max(r["peak_bytes"] for r in v) / 2 ** 20)
    res["config"] = dict(frames=a.frames, window=a.window, levels=a.levels, rounds=a.rounds, size=[H, W])
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--long-frames", type=int, default=257)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--levels", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--synth_scd", action="store_true", help="only y4m_window, with and without --synth_scd")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="dvie_stream_bench_")
    try:
        run_dir = os.path.join(tmp, "run")
        os.makedirs(os.path.join(run_dir, "checkpoint"))
        torch.manual_seed(1024)
        net = nets.InterNet(types.SimpleNamespace(syn_type="inter", highres_large=False, coarse_model="HRNet",
                                                  precision="bf16"))
        torch.save({"session": 0, "epoch": 2, "coarse_model": net.coarse_model.state_dict()},
                   os.path.join(run_dir, "checkpoint", "InterNet_xs2xs_inter_0_1_0.pth"))
        del net
        dirs = {k: os.path.join(tmp, k) for k in ("png", "y4m", "y4m_long")}
        make_data(dirs["png"], a.frames, True)
        make_data(dirs["y4m"], a.frames, False)
        if a.synth_scd:
            return scd_legs(a, run_dir, dirs["y4m"])
        make_data(dirs["y4m_long"], a.long_frames, False)
        legs = dict(png_whole=(dirs["png"], 0), png_window=(dirs["png"], a.window), y4m_window=(dirs["y4m"], a.window))
        slots = (a.frames - 1) * (1 << a.levels) + 1
        run(run_dir, dirs["y4m"], a.window, a.levels)  # warm-up: code objects, allocator
        runs = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, (data, window) in legs.items():
                runs[k].append(run(run_dir, data, window, a.levels))
        res = {}
        for k, v in runs.items():
            walls = sorted(r["wall_s"] for r in v)
            mid = [r for r in v if r["wall_s"] == walls[len(walls) // 2]][0]
            res[k] = dict(wall_s=walls[len(walls) // 2], runs_wall_s=[r["wall_s"] for r in v],
                          spread=(walls[-1] - walls[0]) / walls[len(walls) // 2], slots=slots,
                          slots_per_s=slots / walls[len(walls) // 2], peak_mib=max(r["peak_bytes"] for r in v) / 2 ** 20,
                          stages_of_median_run=mid["stages"])
        long_slots = (a.long_frames - 1) * (1 << a.levels) + 1
        for k, window in (("y4m_long_window", a.window), ("y4m_long_whole", 0)):
            r = run(run_dir, dirs["y4m_long"], window, a.levels)
            res[k] = dict(frames=a.long_frames, wall_s=r["wall_s"], slots=long_slots, slots_per_s=long_slots / r["wall_s"],
                          peak_mib=r["peak_bytes"] / 2 ** 20, stages=r["stages"])
        res["config"] = dict(frames=a.frames, window=a.window, levels=a.levels, rounds=a.rounds, size=[H, W])
        print(json.dumps(res, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
